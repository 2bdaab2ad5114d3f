"""Every op of the Device interface (csrc/include/gj/device.hpp) against a plain numpy reference written
from its contract comment, on both executors: the host reference executor and the gfx950 kernels.

Buffers are torch tensors on the executor's device, passed by data_ptr().  Every output buffer is
larger than what the op may write and pre-filled with a sentinel: a test asserts the exact values in
the region the op may write and the sentinel everywhere else.  Copy / move / selection ops are
exact, so they are compared with equality."""
import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj

EXEC = [pytest.param("cpu"), pytest.param("gpu", marks=pytest.mark.gpu)]
DTYPES = [torch.float64, torch.float32]
_DT = {torch.float64: "fp64", torch.float32: "fp32"}
_NP = {torch.float64: np.float64, torch.float32: np.float32}
SENT = -777.25  # exact in fp32 and fp64, never produced by the inputs below
_devices = {}

# (p, k, g): one rank that owns everything, an owner, a non-owner, a step without a pivot
OWNERS = [(1, 0, 2), (3, 1, 7), (3, 1, 6), (3, 1, -1)]
PIVOT_REC = np.dtype([("score", "<f8"), ("logical", "<i4"), ("phys", "<i4"), ("valid", "<i4"), ("pad", "<i4")])


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


def _a(t):
    return t.cpu().numpy()


def _rand(shape, dtype, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(_NP[dtype])


def _owned(p, k, g):
    return g >= 0 and g % p == k


# ------------------------------------------------------------------ owner_edits
@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("piece", ["none", "w5", "w2m_eye"])
@pytest.mark.parametrize("p,k,g", OWNERS)
@pytest.mark.parametrize("m,j", [(16, 0), (37, 1), (128, 3)])
def test_owner_edits(ex, dtype, piece, p, k, g, m, j):
    # (128, 3, w2m_eye): 5 m^2 + 2 m^2 + m^2 = 131072 work items against the launch's 65536 threads:
    # the grid-stride loop and all four sections
    nloc, krows = 4, (j + 2) * m
    ldl = nloc * m + 3
    At0 = _rand((krows, ldl), dtype, 1)
    inv0 = _rand((nloc * m * m,), dtype, 2)
    w, col0 = {"none": (0, 0), "w5": (5, 3), "w2m_eye": (2 * m, 1)}[piece]
    ldx, ldd, ld_eye = col0 + w + 5, w + 3, m + 3
    X0 = _rand((nloc * m, ldx), dtype, 3)
    lrow0 = np.full(j * m * m + m + 7, SENT, _NP[dtype])  # room for one K-row too many
    ht0 = np.full(m * m + 7, SENT, _NP[dtype])
    dst0 = np.full((m + 1, ldd), SENT, _NP[dtype])
    eye0 = np.full((m + 1, ld_eye), SENT, _NP[dtype])

    At, inv, X, lrow, ht, dst, eye = (_t(a, ex) for a in (At0, inv0, X0, lrow0, ht0, dst0, eye0))
    phys = _t(np.array([g, 12345], np.int32), ex)
    kw = {}
    if w > 0:
        kw.update(dst=dst.data_ptr(), ldd=ldd, X=X.data_ptr(), ldx=ldx, col0=col0, w=w)
    if piece == "w2m_eye":
        kw.update(eye=eye.data_ptr(), ld_eye=ld_eye)
    _dev(ex).owner_edits(_DT[dtype], At.data_ptr(), ldl, phys.data_ptr(), p, k, j, m, lrow.data_ptr(),
                         ht.data_ptr(), inv.data_ptr(), **kw)

    eAt, eX, elrow, eht, edst, eeye = At0.copy(), X0.copy(), lrow0.copy(), ht0.copy(), dst0.copy(), eye0.copy()
    if _owned(p, k, g):
        b = g // p
        row0 = b * m
        elrow[:j * m * m] = At0[:j * m, row0:row0 + m].reshape(-1)
        eAt[:(j + 1) * m, row0:row0 + m] = 0
        eAt[j * m:(j + 1) * m, row0:row0 + m] = np.eye(m)
        eht[:m * m] = inv0[b * m * m:(b + 1) * m * m]
        if w > 0:
            edst[:m, :w] = X0[row0:row0 + m, col0:col0 + w]
            eX[row0:row0 + m, col0:col0 + w] = 0
        if piece == "w2m_eye":
            eeye[:m, :m] = np.eye(m)
    assert np.array_equal(_a(lrow), elrow)
    assert np.array_equal(_a(At), eAt)
    assert np.array_equal(_a(ht), eht)
    assert np.array_equal(_a(dst), edst)
    assert np.array_equal(_a(X), eX)
    assert np.array_equal(_a(eye), eeye)
    assert np.array_equal(_a(inv), inv0)
    assert _a(phys).tolist() == [g, 12345]


# ------------------------------------------------------------------ take_rows
@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p,k,g", OWNERS)
@pytest.mark.parametrize("w", [0, 1, 100, 300])
@pytest.mark.parametrize("m", [16, 37])
def test_take_rows(ex, dtype, p, k, g, w, m):
    nloc, col0 = 4, 3
    ldx, ldd = col0 + w + 5, w + 3
    X0 = _rand((nloc * m, ldx), dtype, 4)
    dst0 = np.full((m + 1, ldd), SENT, _NP[dtype])
    X, dst = _t(X0, ex), _t(dst0, ex)
    phys = _t(np.array([g], np.int32), ex)
    _dev(ex).take_rows(_DT[dtype], dst.data_ptr(), ldd, X.data_ptr(), ldx, phys.data_ptr(), p, k, col0, w, m)
    eX, edst = X0.copy(), dst0.copy()
    if _owned(p, k, g):
        row0 = (g // p) * m
        edst[:m, :w] = X0[row0:row0 + m, col0:col0 + w]
        eX[row0:row0 + m, col0:col0 + w] = 0
    assert np.array_equal(_a(dst), edst)
    assert np.array_equal(_a(X), eX)


# ------------------------------------------------------------------ sum_slices / zero_unless_owner
COUNTS = [1, 1000, 300001]  # the last one exceeds the launch's 1024 x 256 threads


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nslices", [1, 2, 8])
@pytest.mark.parametrize("count", COUNTS)
def test_sum_slices(ex, dtype, nslices, count):
    # 1, half an ulp of 1 and -1: the rounded sum depends on the order of the additions
    tiny = 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24
    vals = np.array([1.0, tiny, -1.0, 3 * tiny], _NP[dtype])
    src0 = vals[np.random.default_rng(5).integers(0, 4, size=nslices * count + 5)]
    dst0 = np.full(count + 5, SENT, _NP[dtype])
    src, dst = _t(src0, ex), _t(dst0, ex)
    _dev(ex).sum_slices(_DT[dtype], dst.data_ptr(), src.data_ptr(), count, nslices)
    acc = src0[:count].copy()
    for q in range(1, nslices):  # in the op's dtype, in q order
        acc = (acc + src0[q * count:(q + 1) * count]).astype(_NP[dtype])
    exp = dst0.copy()
    exp[:count] = acc
    out = _a(dst)
    assert out.tobytes() == exp.tobytes()
    assert np.array_equal(_a(src), src0)


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p,k,g", OWNERS[1:])
@pytest.mark.parametrize("count", COUNTS)
def test_zero_unless_owner(ex, dtype, p, k, g, count):
    buf0 = _rand((count + 5,), dtype, 6)
    buf0[count:] = SENT
    buf = _t(buf0, ex)
    phys = _t(np.array([g], np.int32), ex)
    _dev(ex).zero_unless_owner(_DT[dtype], buf.data_ptr(), count, phys.data_ptr(), p, k)
    exp = buf0.copy()
    if not _owned(p, k, g):
        exp[:count] = 0
    assert np.array_equal(_a(buf), exp)


# ------------------------------------------------------------------ h_block
@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 16, 37, 300])
def test_h_block(ex, dtype, m):
    ldr = m + 3
    Ht0 = _rand((m, m), dtype, 7)  # asymmetric
    R0 = np.full((m + 1, ldr), SENT, _NP[dtype])
    Ht, R = _t(Ht0, ex), _t(R0, ex)
    _dev(ex).h_block(_DT[dtype], R.data_ptr(), ldr, Ht.data_ptr(), m)
    exp = R0.copy()
    exp[:m, :m] = Ht0.T
    assert np.array_equal(_a(R), exp)


# ------------------------------------------------------------------ widen / upload_convert
def _specials(a):
    a[0, :8] = [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -0.0, 1e39, -1e39, np.nan, 1e-46, 2.0 ** -149]
    a[-1, -1] = 1 + 2.0 ** -24  # round-to-even tie: down to 1
    return a


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
def test_upload_convert(ex, dtype):
    rows, cols, ldx, lds = 37, 515, 517, 520
    src0 = _specials(np.random.default_rng(8).standard_normal((rows + 1, lds)))
    src0[:, cols:] = 5.5
    X0 = np.full((rows + 1, ldx), SENT, _NP[dtype])
    src, X = _t(src0, ex), _t(X0, ex)
    _dev(ex).upload_convert(_DT[dtype], X.data_ptr(), ldx, src.data_ptr(), lds, rows, cols)
    exp = X0.copy()
    with np.errstate(over="ignore"):
        exp[:rows, :cols] = src0[:rows, :cols].astype(_NP[dtype])
    out = _a(X)
    assert out.tobytes() == exp.tobytes()  # bitwise: the sign of -0.0, NaN stays NaN
    if dtype == torch.float32:
        assert out[0, 0] == 1.0 and out[0, 1] == np.float32(1 + 2.0 ** -22) and np.signbit(out[0, 2])
        assert out[0, 3] == np.inf and out[0, 4] == -np.inf and np.isnan(out[0, 5])


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
def test_widen(ex, dtype):
    rows, cols, ldx, ldd = 37, 515, 517, 520
    with np.errstate(over="ignore"):
        X0 = _specials(np.random.default_rng(9).standard_normal((rows + 1, ldx))).astype(_NP[dtype])
    dst0 = np.full((rows + 1, ldd), SENT, np.float64)
    X, dst = _t(X0, ex), _t(dst0, ex)
    _dev(ex).widen(_DT[dtype], dst.data_ptr(), ldd, X.data_ptr(), ldx, rows, cols)
    exp = dst0.copy()
    exp[:rows, :cols] = X0[:rows, :cols].astype(np.float64)
    assert _a(dst).tobytes() == exp.tobytes()


# ------------------------------------------------------------------ add_diag
@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nd", [1, 300])
def test_add_diag(ex, dtype, nd):
    ld, alpha = nd + 3, 0.1  # 0.1 is not an fp32 number: fp32 adds (float)alpha
    A0 = _rand((nd + 1, ld), dtype, 10)
    A = _t(A0, ex)
    _dev(ex).add_diag(_DT[dtype], A.data_ptr(), ld, nd, alpha)
    exp = A0.copy()
    i = np.arange(nd)
    exp[i, i] = A0[i, i] + _NP[dtype](alpha)
    assert exp.dtype == A0.dtype
    assert np.array_equal(_a(A), exp)


# ------------------------------------------------------------------ hash_rows
_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _hash_ref(buf, ld_bytes, width_bytes, rows):
    """gen.hpp hash_term summed over the words of the rows (uint64 wrap-around)."""
    ww = width_bytes // 4
    if rows == 0 or ww == 0:
        return 0
    words = np.stack([buf[r * ld_bytes:r * ld_bytes + width_bytes].view("<u4") for r in range(rows)]).reshape(-1)
    idx = np.arange(rows * ww, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (words.astype(np.uint64) << np.uint64(32)) ^ (idx * np.uint64(0xD1B54A32D192ED03)) ^ np.uint64(0x5851F42D4C957F2D)
        return int(_splitmix64(x).sum(dtype=np.uint64))


def _hash_dev(ex, buf, ld_bytes, width_bytes, rows):
    nparts = _dev(ex).kHashParts
    parts0 = np.full(nparts + 3, -1, np.int64)  # all-ones: a part nobody writes shows in the sum
    b, parts = _t(buf, ex), _t(parts0, ex)
    _dev(ex).hash_rows(b.data_ptr(), ld_bytes, width_bytes, rows, parts.data_ptr())
    out = _a(parts)
    assert (out[nparts:] == -1).all()
    assert np.array_equal(_a(b), buf)
    return sum(int(v) for v in out[:nparts].view(np.uint64)) & _M64


HASH_CASES = [(1, 4, 4), (3, 20, 32), (128, 1024, 4096), (77, 1332, 1600), (0, 64, 64)]


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("rows,width,ld", HASH_CASES)
def test_hash_rows(ex, rows, width, ld):
    # (77, 1332, 1600): 25641 words, more than the launch's 64 x 256 threads; (0, 64, 64): every
    # workgroup still writes its (zero) part
    assert gj.load_native().kHashParts == _dev(ex).kHashParts == 64
    buf = np.random.default_rng(11).integers(0, 256, size=max(rows, 1) * ld + 64, dtype=np.uint8)
    assert _hash_dev(ex, buf, ld, width, rows) == _hash_ref(buf, ld, width, rows)


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("rows,width,ld", [(3, 20, 32), (77, 1332, 1600)])
def test_hash_rows_sensitivity(ex, rows, width, ld):
    buf = np.random.default_rng(12).integers(0, 256, size=rows * ld + 64, dtype=np.uint8)
    h0 = _hash_dev(ex, buf, ld, width, rows)
    assert h0 == _hash_ref(buf, ld, width, rows)
    ww = width // 4

    def word(r, w):
        return slice(r * ld + 4 * w, r * ld + 4 * w + 4)

    # one bit in the first, a middle and the last word
    for r, w in [(0, 0), (rows // 2, ww // 2), (rows - 1, ww - 1)]:
        b = buf.copy()
        b[r * ld + 4 * w + 1] ^= 0x10
        h = _hash_dev(ex, b, ld, width, rows)
        assert h != h0 and h == _hash_ref(b, ld, width, rows)
    # two unequal words of one row swapped; two rows swapped
    b = buf.copy()
    b[word(1, 0)] = [1, 2, 3, 4]
    b[word(1, ww - 1)] = [5, 6, 7, 8]
    h1 = _hash_dev(ex, b, ld, width, rows)
    b2 = b.copy()
    b2[word(1, 0)], b2[word(1, ww - 1)] = b[word(1, ww - 1)], b[word(1, 0)]
    h2 = _hash_dev(ex, b2, ld, width, rows)
    assert h1 != h2 and h2 == _hash_ref(b2, ld, width, rows)
    b3 = buf.copy()
    b3[0:width], b3[(rows - 1) * ld:(rows - 1) * ld + width] = buf[(rows - 1) * ld:(rows - 1) * ld + width], buf[0:width]
    h3 = _hash_dev(ex, b3, ld, width, rows)
    assert h3 != h0 and h3 == _hash_ref(b3, ld, width, rows)
    # the pitch gap and the bytes behind the last row are not part of the hash
    b4 = buf.copy()
    for r in range(rows):
        b4[r * ld + width:(r + 1) * ld] ^= 0xFF
    b4[rows * ld:] ^= 0xFF
    assert _hash_dev(ex, b4, ld, width, rows) == h0


# ------------------------------------------------------------------ partial pivoting ops
def _cand_layout(m, p, k):
    """n with 5 local blocks on rank k of p."""
    Nr = 5 if p == 1 else 15
    return Nr * m, Nr


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("special", ["eq", "below", "inf", "nan"])
@pytest.mark.parametrize("p,k", [(1, 0), (3, 1)])
@pytest.mark.parametrize("m", [4, 37, 128])
def test_candidate_maxabs(ex, dtype, special, p, k, m):
    n, Nr = _cand_layout(m, p, k)
    nblk, thresh = 5, 0.75
    ldl = nblk * m + 3
    Lt0 = (np.random.default_rng(13).uniform(-0.5, 0.5, size=(m + 1, ldl))).astype(_NP[dtype])
    Lt0[m, :] = 1e6  # a row below the panel
    Lt0[:m, nblk * m:] = 1e6  # the pitch gap
    used0 = np.zeros(Nr + 2, np.int32)
    used0[0 * p + k] = 1  # local block 0 is used (and holds large values)
    if p > 1:
        used0[1 * p + 0] = used0[2 * p + 2] = 1  # other ranks' blocks: not this rank's business
    Lt0[:m, 0:m] = 50.0
    Lt0[0, 1 * m] = 3.0  # block 1: the maximum at its first element
    Lt0[m - 1, 3 * m - 1] = 2.5  # block 2: at its last element
    Lt0[m // 2, 3 * m + m // 3] = -4.0  # block 3: a negative value
    below = np.nextafter(_NP[dtype](thresh), _NP[dtype](0))
    if special in ("inf", "nan"):
        Lt0[0, 4 * m] = 2.0  # a finite entry above thresh: the non-finite one alone must invalidate
    Lt0[m // 3, 4 * m + m - 1] = {"eq": -thresh, "below": below, "inf": -np.inf, "nan": np.nan}[special]
    scores0 = np.full(nblk + 2, SENT)
    valid0 = np.full(nblk + 2, 99, np.int32)
    Lt, used, scores, valid = _t(Lt0, ex), _t(used0, ex), _t(scores0, ex), _t(valid0, ex)
    _dev(ex).candidate_maxabs(_DT[dtype], Lt.data_ptr(), ldl, scores.data_ptr(), valid.data_ptr(),
                              used.data_ptr(), n, m, p, k, thresh)
    sc, va = _a(scores), _a(valid)
    assert (sc[nblk:] == SENT).all() and (va[nblk:] == 99).all()
    assert va[:4].tolist() == [0, 1, 1, 1]
    assert sc[:4].tolist() == [0.0, -3.0, -2.5, -4.0]
    if special == "eq":
        assert va[4] == 1 and sc[4] == -thresh
    elif special == "below":
        assert va[4] == 0 and sc[4] == -float(below)
    elif special == "inf":
        assert va[4] == 0 and sc[4] == -np.inf
    else:  # a NaN entry makes the candidate invalid, whatever its score
        assert va[4] == 0


def _rec(score, logical, phys, valid, pad=0):
    r = np.zeros(2, PIVOT_REC)
    r[0] = (score, logical, phys, valid, pad)
    r[1] = (SENT, 7, 7, 7, 7)
    return r


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ok", [True, False])
@pytest.mark.parametrize("p,k", [(1, 0), (3, 1)])
@pytest.mark.parametrize("m", [4, 37])
def test_gather_candidate(ex, dtype, ok, p, k, m):
    n, Nr = _cand_layout(m, p, k)
    nblk, b = 5, 2
    ldl = nblk * m + 3
    Lt0 = _rand((m, ldl), dtype, 14)
    sel0 = np.full(m * m + 5, SENT, _NP[dtype])
    rec0 = _rec(-1.5, 4, b * p + k, 1) if ok else _rec(0.0, -1, -1, 0)
    Lt, sel, rec = _t(Lt0, ex), _t(sel0, ex), _t(rec0.view(np.uint8), ex)
    _dev(ex).gather_candidate(_DT[dtype], sel.data_ptr(), Lt.data_ptr(), ldl, rec.data_ptr(), n, m, p, k)
    exp = sel0.copy()
    exp[:m * m] = (Lt0[:, b * m:(b + 1) * m] if ok else -np.eye(m)).reshape(-1)
    assert np.array_equal(_a(sel), exp)
    assert _a(rec).tobytes() == rec0.tobytes()


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("growth", ["off", "passed", "exceeded", "nan"])
@pytest.mark.parametrize("valid1", [1, 0])
@pytest.mark.parametrize("rec_valid", [1, 0])
@pytest.mark.parametrize("m,p,k", [(4, 1, 0), (37, 3, 1)])
def test_commit_candidate(ex, dtype, growth, valid1, rec_valid, m, p, k):
    n, Nr = _cand_layout(m, p, k)
    nblk, b = 5, 2
    # growth estimate = score1 * -rec.score = 3 * 2 = 6: a bound of exactly 6 passes
    bound = {"off": 0.0, "passed": 6.0, "exceeded": np.nextafter(6.0, 0), "nan": 10.0}[growth]
    score1 = np.array([np.nan if growth == "nan" else 3.0, SENT])
    inv_t0 = np.full((nblk + 1) * m * m, SENT, _NP[dtype])
    inv10 = _rand((m * m + 3,), dtype, 15)
    rec0 = _rec(-2.0, 4, b * p + k, rec_valid, pad=5)
    inv_t, inv1, rec = _t(inv_t0, ex), _t(inv10, ex), _t(rec0.view(np.uint8), ex)
    v1, s1 = _t(np.array([valid1, 99], np.int32), ex), _t(score1, ex)
    _dev(ex).commit_candidate(_DT[dtype], inv_t.data_ptr(), inv1.data_ptr(), v1.data_ptr(), s1.data_ptr(),
                              float(bound), rec.data_ptr(), n, m, p, k)
    passes = bool(rec_valid and valid1 and growth in ("off", "passed"))
    exp = inv_t0.copy()
    erec = rec0.copy()
    if passes:
        exp[b * m * m:(b + 1) * m * m] = inv10[:m * m]
    else:
        erec["valid"][0] = 0
    assert np.array_equal(_a(inv_t), exp)
    assert _a(rec).tobytes() == erec.tobytes()
    assert _a(v1).tolist() == [valid1, 99]


# ------------------------------------------------------------------ norms and the residual
BIG = {torch.float64: 1e300, torch.float32: 1e30}  # padding filler (1e300 is not an fp32 number)
U = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23}
NORM_LAYOUTS = [(250, 64, 3, 1), (250, 64, 3, 0), (250, 64, 1, 0)]  # rank 0 of 3 owns the padded block row


def _layout(n, m, p, k):
    Nr = -(-n // m)
    blocks = [b for b in range(Nr) if b % p == k]
    grow = np.concatenate([np.arange(b * m, (b + 1) * m) for b in blocks])  # global row of each local row
    return Nr * m, grow


def _call_norm(ex, dtype, name, X0, n, m, p, k):
    X = _t(X0, ex)
    out = _t(np.array([SENT, SENT]), ex)
    getattr(_dev(ex), name)(_DT[dtype], X.data_ptr(), X0.shape[1], n, m, p, k, out.data_ptr())
    o = _a(out)
    assert o[1] == SENT
    return float(o[0])


def _norm_input(dtype, n, m, p, k, seed):
    """Local rows (ld > npad), padding rows and padding columns full of BIG; the numpy fp64 row sums."""
    npad, grow = _layout(n, m, p, k)
    X0 = _rand((len(grow), npad + 3), dtype, seed)
    X0[:, n:] = BIG[dtype]
    X0[grow >= n, :] = BIG[dtype]
    return X0, grow


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,p,k", NORM_LAYOUTS)
def test_row_abs_max_layouts(ex, dtype, n, m, p, k):
    X0, grow = _norm_input(dtype, n, m, p, k, 16)
    real = grow < n
    Xd = X0[real, :n].astype(np.float64)
    ref = np.abs(Xd).sum(1).max()
    got = _call_norm(ex, dtype, "row_abs_max", X0, n, m, p, k)
    assert abs(got - ref) <= n * 2.0 ** -52 * ref, (got, ref)
    # minus_i: the identity sits on the GLOBAL row index
    D = Xd.copy()
    D[np.arange(real.sum()), grow[real]] -= 1.0
    ref_i = np.abs(D).sum(1).max()
    X1 = X0.copy()
    # make the row of the maximum depend on where the identity lands: a large diagonal entry
    r = int(np.flatnonzero(real)[5])
    X1[r, grow[r]] = 40.0
    D1 = X1[real, :n].astype(np.float64)
    D1[np.arange(real.sum()), grow[real]] -= 1.0
    ref_i1 = np.abs(D1).sum(1).max()
    for Xc, rf in ((X0, ref_i), (X1, ref_i1)):
        got = _call_norm(ex, dtype, "row_abs_max_minus_i", Xc, n, m, p, k)
        assert abs(got - rf) <= n * 2.0 ** -52 * rf, (got, rf)


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["row_abs_max", "row_abs_max_minus_i"])
def test_norm_nan_propagates(ex, dtype, name):
    n, m, p, k = 250, 64, 3, 0  # local blocks 0 and 3: rows 122.. of the second are padding
    X0, grow = _norm_input(dtype, n, m, p, k, 17)
    real = grow < n
    Xd = X0[real, :n].astype(np.float64)
    if name == "row_abs_max_minus_i":
        Xd[np.arange(real.sum()), grow[real]] -= 1.0
    ref = np.abs(Xd).sum(1).max()
    # NaN in the padding (a padding row, a padding column, the pitch gap): ignored
    Xp = X0.copy()
    Xp[-1, 3] = Xp[5, n + 2] = Xp[7, -1] = np.nan
    got = _call_norm(ex, dtype, name, Xp, n, m, p, k)
    assert abs(got - ref) <= n * 2.0 ** -52 * ref, (got, ref)
    # one NaN in one real row
    for r, c in [(70, 100), (0, 0), (int(np.flatnonzero(real)[-1]), n - 1)]:
        Xn = X0.copy()
        Xn[r, c] = np.nan
        assert np.isnan(_call_norm(ex, dtype, name, Xn, n, m, p, k)), (r, c)


def _call_residual(ex, dtype, A0, F0, n, m, p, k):
    A, F = _t(A0, ex), _t(F0, ex)
    out = _t(np.array([SENT, SENT]), ex)
    _dev(ex).residual(_DT[dtype], A.data_ptr(), F.data_ptr(), n, m, p, k, out.data_ptr())
    o = _a(out)
    assert o[1] == SENT
    return float(o[0])


def _padded(A, npad, dtype):
    """A' = diag(A, I), the engine's padding."""
    n = A.shape[0]
    P = np.eye(npad, dtype=_NP[dtype])
    P[:n, :n] = A
    return P


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,p,k", NORM_LAYOUTS)
def test_residual_layouts(ex, dtype, n, m, p, k):
    # Full is random, not an inverse: the residual is O(n), so the relative check is sharp and a
    # misplaced identity (local instead of global row) or a counted padding entry shows.
    npad, grow = _layout(n, m, p, k)
    big = BIG[dtype]
    real = grow < n
    A0 = _rand((len(grow), npad), dtype, 18)
    F0 = _rand((npad, npad), dtype, 19)
    # padding that must not count: A's padding rows and columns, Full's padding columns; Full's
    # padding rows are 0 in the real columns (Device::residual: the inverse of diag(A, I))
    A0[:, n:] = big
    A0[~real, :] = big
    F0[:, n:] = big
    F0[n:, :n] = 0
    Ad, Fd = A0[real, :n].astype(np.float64), F0[:n, :n].astype(np.float64)
    R = Ad @ Fd
    R[np.arange(real.sum()), grow[real]] -= 1.0
    ref = np.abs(R).sum(1).max()
    S = np.abs(Ad) @ np.abs(Fd)
    S[np.arange(real.sum()), grow[real]] += 1.0
    bound = 2 * n * U[dtype] * S.sum(1).max()  # fp32: the GPU's products accumulate in fp32
    got = _call_residual(ex, dtype, A0, F0, n, m, p, k)
    assert abs(got - ref) <= bound, (got, ref, bound)


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["identity_one_nan", "all_nan_24_rows", "nan_row_of_a", "inf_in_full"])
def test_residual_nonfinite_propagates(ex, dtype, case):
    rng = np.random.default_rng(20)
    if case == "identity_one_nan":  # A = I, Full = I with one NaN
        n, m = 8, 4
        A0, F0 = np.eye(n, dtype=_NP[dtype]), np.eye(n, dtype=_NP[dtype])
        F0[3, 2] = np.nan
    elif case == "all_nan_24_rows":  # fewer local rows than one wave
        n, m = 20, 8
        A0 = _padded(rng.standard_normal((n, n)), 24, dtype)
        F0 = np.full((24, 24), np.nan, _NP[dtype])
    else:
        n, m = 250, 64
        A0 = _padded(rng.standard_normal((n, n)), 256, dtype)
        F0 = _padded(rng.standard_normal((n, n)), 256, dtype)
        if case == "nan_row_of_a":  # one NaN row sum among finite ones of the same wave
            A0[100, 7] = np.nan
        else:
            F0[5, 9] = np.inf
    got = _call_residual(ex, dtype, A0, F0, n, m, 1, 0)
    if case == "inf_in_full":
        assert got == np.inf
    else:
        assert np.isnan(got), got


# ------------------------------------------------------------------ block_inverse: non-finite candidates
# (kernel family, m, dtypes): every family of the GPU over its own m range (the host executor has one
# implementation and runs the same shapes)
BI_FAMILIES = [("panel", 17, DTYPES), ("panel", 128, DTYPES), ("sweep", 64, DTYPES), ("co", 64, [torch.float64]),
               ("panel", 200, [torch.float64]),  # the L2-image family
               ("generic", 300, DTYPES), ("blocked", 300, DTYPES), ("huge", 300, DTYPES)]
BI_CASES = [pytest.param(v, m, dt, id=f"{v}-{m}-{_DT[dt]}") for v, m, dts in BI_FAMILIES for dt in dts]
BI_BAD = {1: "nan_5_7", 3: "inf_3_0", 5: "inf_last_col", 7: "overflow"}


def _bi_blocks(m, dtype, base, with_bad):
    """Nine candidates: well-conditioned blocks (dense: randn + 2 sqrt(m) I; diag: 5 I, where a NaN stays
    in one row of the sweep instead of flooding the block) and, with_bad, four broken ones between
    them (Device::block_inverse: a non-finite entry, or a sweep that produces one)."""
    rng = np.random.default_rng(100 + m)
    nblk = 9
    if base == "dense":
        W = rng.standard_normal((nblk, m, m)) + 2.0 * np.sqrt(m) * np.eye(m)
    else:
        W = np.broadcast_to(5.0 * np.eye(m), (nblk, m, m)).copy()
    if with_bad:
        big, small, tiny = (1e200, 1e-199, 1e-200) if dtype == torch.float64 else (1e20, 1e-19, 1e-20)
        W[1][5, 7] = np.nan
        W[3][3, 0] = np.inf
        W[5][2, m - 1] = np.inf
        # column 0 offers only rows 0 and 1: the pivot small, its reciprocal times `big` overflows
        W[7][:2, :] = 0.0
        W[7][:, :2] = 0.0
        W[7][:2, :2] = [[small, big], [tiny, 1.0]]
    return W.astype(_NP[dtype])


def _bi_run(ex, dtype, W, thresh):
    nblk, m = W.shape[0], W.shape[1]
    Lt = _t(-W.reshape(nblk * m, m).T, ex)
    inv_t = _t(np.full((nblk, m, m), SENT, _NP[dtype]), ex)
    scores = _t(np.full(nblk, SENT, np.float64), ex)
    valid = _t(np.full(nblk, -7, np.int32), ex)
    used = _t(np.zeros(nblk, np.int32), ex)
    _dev(ex).block_inverse(_DT[dtype], Lt.data_ptr(), nblk * m, inv_t.data_ptr(), scores.data_ptr(),
                           valid.data_ptr(), used.data_ptr(), nblk * m, m, 1, 0, thresh, -1)
    return _a(inv_t), _a(scores), _a(valid)


@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("base", ["dense", "diag"])
@pytest.mark.parametrize("variant,m,dtype", BI_CASES)
def test_block_inverse_nonfinite_candidate_is_invalid(ex, base, variant, m, dtype):
    """A candidate that holds a NaN or an Inf, or whose sweep overflows, comes back valid = 0 and
    score = 0 (it must never win the pivot selection with a score that a maximum took from the finite
    rows only); its good neighbours are bit-identical to a launch without the broken blocks."""
    thresh = 1e-300 if dtype == torch.float64 else 1e-30
    C = gj.load_native()
    C.set_block_inverse_variant(variant)
    try:
        inv_b, sc_b, va_b = _bi_run(ex, dtype, _bi_blocks(m, dtype, base, True), thresh)
        inv_g, sc_g, va_g = _bi_run(ex, dtype, _bi_blocks(m, dtype, base, False), thresh)
    finally:
        C.set_block_inverse_variant("panel")
    assert va_g.tolist() == [1] * 9
    got = {name: (int(va_b[b]), float(sc_b[b])) for b, name in BI_BAD.items()}
    assert got == {name: (0, 0.0) for name in BI_BAD.values()}, got
    good = [b for b in range(9) if b not in BI_BAD]
    assert va_b[good].tolist() == [1] * len(good)
    assert np.array_equal(sc_b[good], sc_g[good])
    assert np.array_equal(inv_b[good], inv_g[good])
    assert np.isfinite(inv_b[good]).all() and np.isfinite(sc_b[good]).all()


@pytest.mark.parametrize("ex", EXEC)
def test_ops_wrappers(ex):
    from mpi_jordan_crazy_acceleration_amd import ops
    Ht0 = _rand((37, 37), torch.float64, 22)
    assert np.array_equal(_a(ops.h_block(_t(Ht0, ex), ldr=40)), Ht0.T)
    buf = np.random.default_rng(23).integers(0, 256, size=3 * 32, dtype=np.uint8)
    assert ops.hash_rows(_t(buf, ex), 32, 20, 3) == _hash_ref(buf, 32, 20, 3)
    n, m = 20, 8
    X0 = _padded(_rand((n, n), torch.float64, 24), 24, torch.float64)
    ref = np.abs(X0[:n, :n] - np.eye(n)).sum(1).max()
    assert abs(ops.row_abs_max_minus_i(_t(X0, ex), n, m) - ref) <= n * 2.0 ** -52 * ref


# ------------------------------------------------------------------ scalar agreements
def test_engine_agreements_turn_nan_into_inf():
    # the engine's share of norm_inf / residual_* is +Inf where the device reduction gave NaN, so a
    # MAX all-reduce with any NaN rule (RCCL, gloo) cannot make it finite again
    C = gj.load_native()
    n, m = 8, 4
    eng = C.Engine(C.host_device(1), C.self_comm(), n, m, "fp64")
    A = np.eye(n)
    A[3, 2] = np.nan
    eng.upload_local_rows(A)
    assert eng.norm_inf() == np.inf
    eng.generate("identity", 0)
    assert eng.norm_inf() == 1.0
    assert eng.solve()["status"] == 0
    assert eng.residual_rows(np.eye(n)) == 0.0
    assert eng.residual_rows(A) == np.inf


# ------------------------------------------------------------------ scalar agreement of the loopback ranks
@pytest.mark.parametrize("async_", [False, True])
@pytest.mark.parametrize("p", [2, 4])
def test_loopback_host_max(p, async_):
    C = gj.load_native()
    vals = [float(v) for v in np.random.default_rng(21).standard_normal(p)]
    assert C.loopback_host_max(vals, async_) == [max(vals)] * p
    for pos in range(p):  # a NaN from any rank wins, on every rank
        v = list(vals)
        v[pos] = float("nan")
        got = C.loopback_host_max(v, async_)
        assert len(got) == p and not any(np.isfinite(g) for g in got), (pos, got)
        v[pos] = float("inf")
        assert C.loopback_host_max(v, async_) == [float("inf")] * p
