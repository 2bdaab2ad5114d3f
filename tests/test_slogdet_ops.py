"""Device::slogdet_batch (csrc/include/gj/device.hpp) against its contract, on the host executor and
on the GPU (csrc/kernels/slogdet.hip).

Reference: numpy.linalg.slogdet in fp64 of the block (an fp32 block widened exactly first, as the op
does).  The sign must be equal; |logabs - ref| <= m * cond_inf(block) * 2^-52, the first-order bound
|tr(inv(B) E)| <= m ||inv(B)|| ||E|| for a backward error of one ulp per entry (derived, not measured).

m = 1, 7, 16, 20, 64, 128 run in LDS on the GPU (probe "sld:lds:*"), m = 130 and 256 in global
scratch ("sld:glob:*"); nb = 1 and 3 for every m, nb = 257 at m = 16 (more blocks than CUs) and
nb = 513 at m = 130 (more blocks than the global form launches workgroups: its grid-stride loop).
"""
import functools

import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd import ops

EPS = 2.0 ** -52
DTS = {"fp64": torch.float64, "fp32": torch.float32}
# (130, 513): more blocks than the global form has workgroups (512), so one of them takes a second block
CASES = [(m, nb) for m in (1, 7, 16, 20, 64, 128, 130, 256) for nb in (1, 3)] + [(16, 257), (130, 513)]
SENTINEL = -12345.5


@functools.lru_cache(maxsize=None)
def _blocks(m, nb, dt):
    """random blocks in dtype dt, their fp64 slogdet and the tolerance per block (computed once)"""
    rng = np.random.default_rng(1000 * m + nb)
    B = torch.from_numpy(rng.standard_normal((nb, m, m))).to(DTS[dt])
    wide = B.to(torch.float64).numpy()
    sign, logabs = np.linalg.slogdet(wide)
    tol = np.array([m * np.linalg.cond(wide[b], np.inf) * EPS for b in range(nb)])
    return B, sign, logabs, tol


def _probe(device, m, dt):
    name = gj.load_native().last_slogdet_kernel()
    if device == "cpu":
        assert name == "host", name
    else:
        assert name == f"sld:{'lds' if m <= 128 else 'glob'}:{'f64' if dt == 'fp64' else 'f32'}", name


def _random_case(device, m, nb, dt):
    B, rs, rl, tol = _blocks(m, nb, dt)
    Bd = B.to(device)
    keep = Bd.clone()
    s, l = ops.slogdet_batch(Bd)
    _probe(device, m, dt)
    assert s.dtype == l.dtype == torch.float64 and s.device == Bd.device
    s, l = s.cpu().numpy(), l.cpu().numpy()
    err = np.abs(l - rl)
    print(f"m={m} nb={nb} {dt}: max |dlog| = {err.max():.3e}, smallest bound {tol.min():.3e}")
    assert np.array_equal(s, rs), (s, rs)
    assert (err <= tol).all(), (err, tol)
    assert torch.equal(Bd.view(torch.uint8), keep.view(torch.uint8))  # the input is only read
    s2, l2 = ops.slogdet_batch(Bd)  # no atomics: the same bits again
    assert np.array_equal(s2.cpu().numpy().view(np.uint64), s.view(np.uint64))
    assert np.array_equal(l2.cpu().numpy().view(np.uint64), l.view(np.uint64))


def _special_case(device, m, dt):
    """one launch: [odd permutation, random, two equal rows, one NaN, random, one Inf]; the random blocks
    must come out as they do alone"""
    B, rs, rl, tol = _blocks(m, 3, dt)
    perm = torch.eye(m, dtype=DTS[dt])
    perm[[0, m - 1]] = perm[[m - 1, 0]].clone()  # one transposition
    twin = B[2].clone()
    twin[m - 1] = twin[m // 2]
    nan = B[1].clone()
    nan[m // 3, m - 1] = float("nan")
    inf = B[0].clone()
    inf[m - 1, 0] = float("inf")
    batch = torch.stack([perm, B[0], twin, nan, B[1], inf]).contiguous().to(device)
    s, l = ops.slogdet_batch(batch)
    _probe(device, m, dt)
    s, l = s.cpu().numpy(), l.cpu().numpy()
    assert s[0] == -1.0 and l[0] == 0.0 and not np.signbit(l[0]), (s[0], l[0])
    assert s[2] == 0.0 and l[2] == -np.inf, (s[2], l[2])
    assert np.isnan(s[3]) and np.isnan(l[3]), (s[3], l[3])
    assert np.isnan(s[5]) and np.isnan(l[5]), (s[5], l[5])
    alone_s, alone_l = ops.slogdet_batch(B[:2].contiguous().to(device))
    assert np.array_equal(s[[1, 4]].view(np.uint64), alone_s.cpu().numpy().view(np.uint64))
    assert np.array_equal(l[[1, 4]].view(np.uint64), alone_l.cpu().numpy().view(np.uint64))
    assert np.array_equal(s[[1, 4]], rs[:2]) and (np.abs(l[[1, 4]] - rl[:2]) <= tol[:2]).all()


def _which_case(device, m, dt):
    B, rs, rl, tol = _blocks(m, 3, dt)
    Bd = B.to(device)
    which = torch.tensor([1, 0, 1], dtype=torch.int32, device=device)
    s = torch.full((3,), SENTINEL, dtype=torch.float64, device=device)
    l = torch.full((3,), SENTINEL, dtype=torch.float64, device=device)
    ops.slogdet_batch(Bd, which=which, sign=s, logabs=l)
    s, l = s.cpu().numpy(), l.cpu().numpy()
    assert s[1] == SENTINEL and l[1] == SENTINEL  # skipped: left untouched
    assert np.array_equal(s[[0, 2]], rs[[0, 2]]) and (np.abs(l[[0, 2]] - rl[[0, 2]]) <= tol[[0, 2]]).all()
    none = torch.zeros(3, dtype=torch.int32, device=device)
    s = torch.full((3,), SENTINEL, dtype=torch.float64, device=device)
    ops.slogdet_batch(Bd, which=none, sign=s, logabs=s.clone())
    assert (s.cpu().numpy() == SENTINEL).all()


_ids = lambda c: f"m{c[0]}-nb{c[1]}"  # noqa: E731
_SPECIAL_M = [7, 16, 20, 128, 130]


@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_slogdet_batch_host(case, dt):
    _random_case("cpu", case[0], case[1], dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_slogdet_batch_gpu(case, dt):
    _random_case("cuda", case[0], case[1], dt)


@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("m", _SPECIAL_M)
def test_slogdet_batch_special_host(m, dt):
    _special_case("cpu", m, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("m", _SPECIAL_M)
def test_slogdet_batch_special_gpu(m, dt):
    _special_case("cuda", m, dt)


@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("m", [16, 130])
def test_slogdet_batch_which_host(m, dt):
    _which_case("cpu", m, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("m", [16, 130])
def test_slogdet_batch_which_gpu(m, dt):
    _which_case("cuda", m, dt)


def _nonfinite_behind_zero_case(device, m, dt):
    """a NaN or an Inf gives (NaN, NaN) also where an exactly zero pivot would come first: column 0 all
    zeros and the entry in a later column, in its last row and column, and in column 0 itself"""
    B = _blocks(m, 3, dt)[0]
    out = []
    for bad in (float("nan"), float("inf"), float("-inf")):
        for r, c in ((m // 2, m - 1), (m - 1, m - 1), (0, 1)):
            blk = B[0].clone()
            blk[:, 0] = 0.0
            blk[r, c] = bad
            out.append(blk)
    zero = B[1].clone()
    zero[:, 0] = 0.0  # and without such an entry the zero column still gives (0, -inf)
    out.append(zero)
    s, l = ops.slogdet_batch(torch.stack(out).contiguous().to(device))
    s, l = s.cpu().numpy(), l.cpu().numpy()
    assert np.isnan(s[:-1]).all() and np.isnan(l[:-1]).all(), (s, l)
    assert s[-1] == 0.0 and l[-1] == -np.inf


@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("m", [7, 128, 130])
def test_slogdet_batch_nonfinite_behind_zero_host(m, dt):
    _nonfinite_behind_zero_case("cpu", m, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("m", [7, 128, 130])
def test_slogdet_batch_nonfinite_behind_zero_gpu(m, dt):
    _nonfinite_behind_zero_case("cuda", m, dt)


def test_slogdet_batch_one_by_one_host():
    """m = 1: the entry itself; zero, negative zero and a negative entry"""
    B = torch.tensor([[[2.0]], [[-0.5]], [[0.0]], [[-0.0]]], dtype=torch.float64)
    s, l = ops.slogdet_batch(B)
    assert s.tolist() == [1.0, -1.0, 0.0, 0.0]
    assert l[2:].tolist() == [-np.inf, -np.inf]
    assert np.abs(l[:2].numpy() - np.log([2.0, 0.5])).max() <= EPS


@pytest.mark.gpu
def test_slogdet_batch_gpu_tied_pivots():
    """equal magnitudes in a column: a matrix of +-1 makes the whole first column one tie (and later
    columns tie often); the arg-max must still settle on one row on every lane"""
    rng = np.random.default_rng(5)
    B = torch.from_numpy(np.sign(rng.standard_normal((3, 20, 20))))
    sh, lh = ops.slogdet_batch(B)
    sg, lg = ops.slogdet_batch(B.cuda())
    rs, rl = np.linalg.slogdet(B.numpy())
    assert np.array_equal(sh.numpy(), rs) and np.array_equal(sg.cpu().numpy(), rs)
    assert np.abs(lg.cpu().numpy() - lh.numpy()).max() <= 1e-12
