"""The pivot selection fused into the candidate-inverse launch (Device::block_inverse_select; on the GPU
select_tail of csrc/kernels/pivot_select.hpp, run by the last workgroup of blockinv_mfma.hip and of the
co-resident kernel of blockinv_big.hip), driven directly, on both executors.

The reference is the pivot rule itself: the minimum ||inv(candidate)||_inf, exact ties to the larger
rank (logical % p), then to the smaller local row (logical / p), with ||inv||_inf from a plain numpy
longdouble Gauss-Jordan on the values the kernel sees (after the cast to the tested dtype).  The
candidates are scaled so that their reference scores are at least 5 % apart (asserted on the
reference alone): with test_block_inverse's tolerances (1e-8 fp64, 2e-2 fp32, relative) the order of the
kernel's scores is then the reference's, and a selection that is valid but not minimal fails."""
import functools

import numpy as np
import pytest
import torch

import mpi_jordan_crazy_acceleration_amd as gj
from mpi_jordan_crazy_acceleration_amd import ops

EXEC = [pytest.param("cpu"), pytest.param("gpu", marks=pytest.mark.gpu)]
_NP = {torch.float64: np.float64, torch.float32: np.float32}
_TOL = {torch.float64: 1e-8, torch.float32: 2e-2}
THRESH = 1e-12
PIVOT_REC = np.dtype([("score", "<f8"), ("logical", "<i4"), ("phys", "<i4"), ("valid", "<i4"), ("pad", "<i4")])
PIVOT_RESULT = np.dtype([("found", "<i4"), ("phys", "<i4"), ("owner", "<i4"), ("logical", "<i4"),
                         ("score", "<f8"), ("step", "<i4"), ("pad", "<i4")])
GUARD = 3           # elements behind every int32 array that nothing may write
I_SENT = -5         # int32 sentinel
B_SENT = 0xAB       # byte sentinel of the 32-byte records
F_SENT = -777.25    # exact in fp32 and fp64
INVALID = (0.0, -1, -1, 0, 0)  # pivot_invalid() (gj/pivot.hpp)

# (variant, dtype, m, nblk): nblk = 70: a lane of the selecting wave scans two candidates, and
# live_block reaches its second ballot; "co": the co-resident kernel (fp64, 32 < m <= 128)
CHAIN = ([("panel", dt, m, 6) for dt in (torch.float64, torch.float32) for m in (17, 32, 33, 64, 100, 128)]
         + [("panel", dt, m, 70) for dt in (torch.float64, torch.float32) for m in (17, 33)]
         + [("co", torch.float64, m, 6) for m in (33, 64, 100, 128)])
RANKS = ([("panel", dt, m, nblk) for dt in (torch.float64, torch.float32) for m, nblk in ((17, 70), (64, 6), (128, 6))]
         + [("co", torch.float64, 64, 6)])


def _id(c):
    return f"{c[0]}-{'fp64' if c[1] == torch.float64 else 'fp32'}-m{c[2]}-nblk{c[3]}"


# ------------------------------------------------------------------ the reference
def _ref_inverse(W):
    """Gauss-Jordan with partial pivoting in longdouble: (inverse, ||inverse||_inf), or None when a
    pivot falls below THRESH (Device::block_inverse's singularity test)."""
    m = W.shape[0]
    A = W.astype(np.longdouble)
    inv = np.eye(m, dtype=np.longdouble)
    for k in range(m):
        r = k + int(np.argmax(np.abs(A[k:, k])))
        if not abs(A[r, k]) >= THRESH:
            return None
        A[[k, r]] = A[[r, k]]
        inv[[k, r]] = inv[[r, k]]
        d = A[k, k]
        A[k] /= d
        inv[k] /= d
        f = A[:, k].copy()
        f[k] = 0
        A -= np.outer(f, A[k])
        inv -= np.outer(f, inv[k])
    return inv, np.abs(inv).sum(axis=1).max()


@functools.lru_cache(maxsize=None)
def _candidates(m, nblk, dtype, ntie):
    """nblk candidates (as the tested dtype holds them) and their reference: well-conditioned random
    blocks scaled onto a shuffled 10 % ladder of scores, among them an all-zero block (1), a block
    that goes singular half-way through the sweep (3) and `ntie` bit-identical blocks (the last of
    them is block 2, the others block 4, 5, ...).  Returns (W, ref) with ref[b] = (inverse, score) or
    None.  Shared by every test of one shape and never modified."""
    rng = np.random.default_rng(1000 * m + nblk)
    W = rng.standard_normal((nblk, m, m)) + 2.0 * np.sqrt(m) * np.eye(m)
    ties = [2] + list(range(4, 4 + ntie - 1))
    ladder = rng.permutation(nblk)
    if ntie == 3:
        ladder[ladder.tolist().index(0)], ladder[2] = ladder[2], 0  # the tied blocks hold the minimum
    for b in range(nblk):
        W[b] *= float(_ref_inverse(W[b])[1]) / (0.1 * 1.1 ** ladder[b])
    for b in ties[1:]:
        W[b] = W[2]
    W[1] = 0.0
    W[3][:, m // 2] = 0.0
    W = W.astype(_NP[dtype])
    W.setflags(write=False)
    ref = [_ref_inverse(W[b].astype(np.float64)) for b in range(nblk)]
    assert ref[1] is None and ref[3] is None and all(ref[b] is not None for b in range(nblk) if b not in (1, 3))
    distinct = np.sort(np.array([float(ref[b][1]) for b in range(nblk) if b not in (1, 3) and b not in ties[1:]]))
    assert (distinct[1:] / distinct[:-1]).min() >= 1.05, distinct
    assert all(ref[b][1] == ref[2][1] for b in ties)
    return W, ref


# ------------------------------------------------------------------ buffers
def _t(arr, ex):
    t = torch.from_numpy(np.ascontiguousarray(arr)).clone()
    if ex == "gpu":
        t = t.cuda()
        torch.cuda.synchronize()
    return t


def _a(t):
    return t.cpu().numpy().copy()


def _i32(values, ex):
    return _t(np.concatenate([np.asarray(values, np.int32), np.full(GUARD, I_SENT, np.int32)]), ex)


class Buffers:
    """Every buffer of one block_inverse_select call, pre-filled: the candidates' outputs and the
    records with sentinels, the book-keeping with the caller's state."""

    def __init__(self, ex, dtype, Wloc, Nr, pos, used, done=0):
        nblk, m = Wloc.shape[0], Wloc.shape[1]
        self.ex, self.dtype, self.m, self.nblk, self.Nr = ex, dtype, m, nblk, Nr
        self.Lt = _t(-Wloc.reshape(nblk * m, m).T, ex)  # K-major panel: W_b = -(Lt block b)^T
        self.inv_t = _t(np.full((nblk, m, m), F_SENT, _NP[dtype]), ex)
        self.scores = _t(np.full(nblk + GUARD, F_SENT, np.float64), ex)
        self.valid = _i32(np.full(nblk, I_SENT), ex)
        phys_at = np.empty(Nr, np.int32)
        phys_at[np.asarray(pos)] = np.arange(Nr, dtype=np.int32)
        self.pos, self.phys_at, self.used = _i32(pos, ex), _i32(phys_at, ex), _i32(used, ex)
        self.seq = _i32(np.full(Nr, I_SENT), ex)
        self.rec = _t(np.full(32 + 16, B_SENT, np.uint8), ex)
        self.out = _t(np.full(32 + 16, B_SENT, np.uint8), ex)
        self.done = _i32([done], ex)

    def select(self, p, k, nlive, t):
        return ops.block_inverse_select(self.Lt, self.inv_t, self.scores, self.valid, self.used, self.Nr * self.m,
                                        self.m, p, k, THRESH, nlive, t, self.pos, self.phys_at, self.seq, self.rec,
                                        self.out, self.done)

    def plain(self, p, k, nlive, used, inv_t, scores, valid):
        """Device::block_inverse of the same kernel family into copies of the pre-launch outputs."""
        out = [_t(inv_t, self.ex), _t(scores, self.ex), _t(valid, self.ex)]
        u = _t(used, self.ex)
        ops.device_for(self.Lt).block_inverse(ops._DT[self.dtype], self.Lt.data_ptr(), self.Lt.stride(0),
                                              out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), u.data_ptr(),
                                              self.Nr * self.m, self.m, p, k, THRESH, nlive)
        if self.ex == "gpu":
            torch.cuda.synchronize()
        return [_a(x) for x in out]

    def state(self):
        names = ("inv_t", "scores", "valid", "pos", "phys_at", "used", "seq", "rec", "out", "done")
        if self.ex == "gpu":
            torch.cuda.synchronize()
        return {n: _a(getattr(self, n)) for n in names}


@pytest.fixture
def variant(request):
    C = gj.load_native()
    C.set_block_inverse_variant(request.param)
    yield request.param
    C.set_block_inverse_variant("panel")


# ------------------------------------------------------------------ the rule, in Python
def _better(a, b, p):
    """pivot_better (gj/pivot.hpp) on (score, logical, phys, valid, pad) tuples."""
    if not a[3]:
        return False
    if not b[3]:
        return True
    if a[0] != b[0]:
        return a[0] < b[0]
    ra, rb = a[1] % p, b[1] % p
    if ra != rb:
        return ra > rb
    return a[1] // p < b[1] // p


def _argmin(scores, valid, used, pos, nblk, p, k):
    best = INVALID
    for b in range(nblk):
        g = b * p + k
        if used[g] or not valid[b]:
            continue
        c = (float(scores[b]), int(pos[g]), g, 1, 0)
        if _better(c, best, p):
            best = c
    return best


def _rec_bytes(rec):
    """The 24 bytes of PivotRec's fields (the struct is padded to 32: its last 8 bytes carry nothing)."""
    return np.frombuffer(np.array([rec], dtype=PIVOT_REC).tobytes(), np.uint8)


def _result_bytes(best, t, p):
    r = (1, best[2], best[2] % p, best[1], best[0], t, 0) if best[3] else (0, -1, -1, -1, 0.0, t, 0)
    return np.frombuffer(np.array([r], dtype=PIVOT_RESULT).tobytes(), np.uint8), r


def _show(raw, dtype):
    return np.frombuffer(raw[:dtype.itemsize].tobytes(), dtype)[0]


def _commit(t, s, pos, phys_at, used, seq):
    """pivot_commit (gj/pivot.hpp)."""
    q, ls = phys_at[t], pos[s]
    pos[q] = ls
    phys_at[ls] = q
    pos[s] = t
    phys_at[t] = s
    used[s] = 1
    seq[t] = s


def _sentinel_tail(st):
    assert (st["rec"][32:] == B_SENT).all() and (st["out"][32:] == B_SENT).all()
    for n in ("valid", "pos", "phys_at", "used", "seq", "done"):
        assert (st[n][-GUARD:] == I_SENT).all(), n
    assert (st["scores"][-GUARD:] == F_SENT).all()


def _check_outputs_against_plain(ex, buf, before, st, p, k, nlive):
    """scores / valid / inv_t of the live blocks: bit-equal to Device::block_inverse of the same family
    from the same state.  Used blocks: untouched on the GPU (no workgroup is dispatched for them),
    valid = 0 / score = 0 on the host executor, which visits every block."""
    inv_p, sc_p, va_p = buf.plain(p, k, nlive, before["used"], before["inv_t"], before["scores"], before["valid"])
    assert np.array_equal(st["valid"], va_p)
    assert np.array_equal(st["scores"].view(np.int64), sc_p.view(np.int64))
    assert st["inv_t"].tobytes() == inv_p.tobytes()
    for b in range(buf.nblk):
        if before["used"][b * p + k]:
            if ex == "gpu":
                assert st["valid"][b] == before["valid"][b] and st["scores"][b] == before["scores"][b]
                assert np.array_equal(st["inv_t"][b], before["inv_t"][b])
            else:
                assert (st["valid"][b], st["scores"][b]) == (0, 0.0)


# ------------------------------------------------------------------ the chain at p = 1
@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("variant,dtype,m,nblk", [pytest.param(*c, id=_id(c)) for c in CHAIN], indirect=["variant"])
def test_fused_selection_chain_single_rank(ex, variant, dtype, m, nblk):
    """t = 0 .. nblk-1, one fused launch per step with nlive = nblk - t; the used flags evolve only through
    the kernel's own book-keeping."""
    W, ref = _candidates(m, nblk, dtype, 2)
    # logical != physical; the tied pair: block 2 at the last logical position, block 4 right before
    # it, so the pair is decided against the physical order, and no step's swap moves either of them
    # before it is chosen (a swap only moves the row at logical position t < the number of valid blocks)
    rest = [b for b in range(nblk) if b not in (2, 4)]
    perm = np.random.default_rng(m + nblk).permutation(nblk - 2)
    pos = np.empty(nblk, np.int32)
    pos[rest] = perm
    pos[4], pos[2] = nblk - 2, nblk - 1
    buf = Buffers(ex, dtype, W, nblk, pos, np.zeros(nblk, np.int32))
    st = buf.state()
    h_pos, h_phys, h_used, h_seq = (st[n][:nblk].tolist() for n in ("pos", "phys_at", "used", "seq"))
    assert h_pos != list(range(nblk))
    chosen = []
    for t in range(nblk):
        before = st
        fused, mirror = buf.select(1, 0, nblk - t, t)
        assert fused is True
        st = buf.state()
        _sentinel_tail(st)
        _check_outputs_against_plain(ex, buf, before, st, 1, 0, nblk - t)
        if t == 0:  # the values, once: against the longdouble reference
            for b in range(nblk):
                assert st["valid"][b] == (ref[b] is not None), b
                if ref[b] is None:
                    continue
                inv, score = ref[b]
                got = st["inv_t"][b].astype(np.float64).T
                assert np.abs(got - inv).max() / np.abs(inv).max() < _TOL[dtype], b
                assert abs(st["scores"][b] - score) / score < _TOL[dtype], b
        best = _argmin(st["scores"], st["valid"], h_used, h_pos, nblk, 1, 0)
        assert np.array_equal(st["rec"][:24], _rec_bytes(best)), (t, _show(st["rec"], PIVOT_REC), best)
        want_out, r = _result_bytes(best, t, 1)
        assert np.array_equal(st["out"][:32], want_out), (t, _show(st["out"], PIVOT_RESULT), r)
        assert mirror == (t, r[0], r[1], r[2], r[3], r[4])
        if best[3]:
            chosen.append(best[2])
            _commit(t, best[2], h_pos, h_phys, h_used, h_seq)
        else:  # only singular blocks are left: nothing found, the book-keeping stays
            h_seq[t] = -1
            assert mirror[1] == 0 and st["seq"][t] == -1
            for n in ("pos", "phys_at", "used"):
                assert np.array_equal(st[n], before[n]), n
        assert st["pos"][:nblk].tolist() == h_pos and st["phys_at"][:nblk].tolist() == h_phys
        assert st["used"][:nblk].tolist() == h_used and st["seq"][:nblk].tolist() == h_seq
        assert st["done"][0] == 0
    # the whole chain: ascending reference scores, the tied pair by logical position (4 before 2)
    order = sorted((b for b in range(nblk) if ref[b] is not None), key=lambda b: (float(ref[b][1]), -b))
    assert chosen == order
    assert chosen.index(4) + 1 == chosen.index(2)
    assert h_seq[len(order):] == [-1] * (nblk - len(order)) and sorted(np.flatnonzero(h_used)) == sorted(order)


# ------------------------------------------------------------------ p > 1: the local argmin only
@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("p,k", [(3, 1), (4, 3)])
@pytest.mark.parametrize("variant,dtype,m,nblk", [pytest.param(*c, id=_id(c)) for c in RANKS], indirect=["variant"])
def test_fused_selection_local_record_many_ranks(ex, variant, dtype, m, nblk, p, k):
    """p > 1: the launch's last workgroup writes this rank's record and nothing else.  Three
    bit-identical candidates hold the minimum: the larger logical % p wins, then the smaller logical / p."""
    W, ref = _candidates(m, nblk, dtype, 3)
    Nr = nblk * p
    rng = np.random.default_rng(7 * m + p)
    used = (rng.random(Nr) < 0.4).astype(np.int32)
    tied = [b * p + k for b in (2, 4, 5)]  # block 5 must win
    used[tied] = 0
    # block 2: the smallest logical position of all, but rank 0; blocks 4 and 5: rank p - 1, block 5
    # on the smaller local row
    want = {tied[0]: 0, tied[1]: 2 * p + p - 1, tied[2]: p + p - 1}
    free = [x for x in rng.permutation(Nr).tolist() if x not in want.values()]
    pos = np.empty(Nr, np.int32)
    for g in range(Nr):
        pos[g] = want[g] if g in want else free.pop()
    assert sorted(pos.tolist()) == list(range(Nr))
    nlive = int((used[k::p] == 0).sum())
    buf = Buffers(ex, dtype, W, Nr, pos, used)
    before = buf.state()
    fused, mirror = buf.select(p, k, nlive, 3)
    assert fused is True and mirror is None
    st = buf.state()
    _sentinel_tail(st)
    _check_outputs_against_plain(ex, buf, before, st, p, k, nlive)
    best = _argmin(st["scores"], st["valid"], used, pos, nblk, p, k)
    assert best[2] == tied[2] and best[0] == st["scores"][2] == st["scores"][4]
    assert np.array_equal(st["rec"][:24], _rec_bytes(best)), (_show(st["rec"], PIVOT_REC), best)
    for n in ("pos", "phys_at", "seq", "out", "used"):  # (used: a required input, so its pre-launch copy)
        assert np.array_equal(st[n], before[n]), n
    assert (st["seq"] == I_SENT).all() and (st["out"] == B_SENT).all()
    assert st["done"][0] == 0


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize("ex", EXEC)
@pytest.mark.parametrize("p,k", [(1, 0), (3, 1)])
@pytest.mark.parametrize("nlive", [0, 1])
@pytest.mark.parametrize("variant,dtype,m", [("panel", torch.float64, 33), ("panel", torch.float32, 128),
                                             ("co", torch.float64, 64)], indirect=["variant"])
def test_fused_selection_no_or_one_live_block(ex, variant, dtype, m, p, k, nlive):
    """nlive = 0: every own row is used, the grid is one workgroup and it has no block; nlive = 1."""
    nblk, t = 6, 4
    W, ref = _candidates(m, nblk, dtype, 2)
    Nr = nblk * p
    rng = np.random.default_rng(m + p + nlive)
    used = (rng.random(Nr) < 0.5).astype(np.int32)
    used[k::p] = 1
    live = 5  # a valid block
    if nlive:
        used[live * p + k] = 0
    pos = rng.permutation(Nr).astype(np.int32)
    buf = Buffers(ex, dtype, W, Nr, pos, used)
    before = buf.state()
    fused, mirror = buf.select(p, k, nlive, t)
    assert fused is True
    st = buf.state()
    _sentinel_tail(st)
    _check_outputs_against_plain(ex, buf, before, st, p, k, nlive)
    best = (float(st["scores"][live]), int(pos[live * p + k]), live * p + k, 1, 0) if nlive else INVALID
    if nlive:
        assert st["valid"][live] == 1 and abs(st["scores"][live] - ref[live][1]) / ref[live][1] < _TOL[dtype]
    assert np.array_equal(st["rec"][:24], _rec_bytes(best)), (_show(st["rec"], PIVOT_REC), best)
    assert st["done"][0] == 0
    if p > 1:
        assert mirror is None
        for n in ("pos", "phys_at", "seq", "out", "used"):
            assert np.array_equal(st[n], before[n]), n
        return
    want_out, r = _result_bytes(best, t, 1)
    assert np.array_equal(st["out"][:32], want_out), (_show(st["out"], PIVOT_RESULT), r)
    assert mirror == (t, r[0], r[1], r[2], r[3], r[4]) and mirror[1] == nlive
    h = {n: before[n][:Nr].tolist() for n in ("pos", "phys_at", "used", "seq")}
    if nlive:
        _commit(t, live, h["pos"], h["phys_at"], h["used"], h["seq"])
    else:
        h["seq"][t] = -1
    for n in h:
        assert st[n][:Nr].tolist() == h[n], n


# ------------------------------------------------------------------ not fusable
NOT_FUSABLE = [pytest.param("cpu", "panel", 16), pytest.param("cpu", "panel", 200),
               pytest.param("gpu", "panel", 16, marks=pytest.mark.gpu),
               pytest.param("gpu", "panel", 200, marks=pytest.mark.gpu),
               # kernel families exist on the GPU only: the host executor has one implementation
               pytest.param("gpu", "sweep", 64, marks=pytest.mark.gpu),
               pytest.param("gpu", "generic", 64, marks=pytest.mark.gpu)]


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("ex,variant,m", NOT_FUSABLE, indirect=["variant"])
def test_not_fusable_enqueues_nothing(ex, variant, m, p):
    """False = the caller runs block_inverse and the selection itself: no output buffer, and not the
    counter either, may have been touched."""
    nblk, dtype = 4, torch.float64
    W = np.random.default_rng(m).standard_normal((nblk, m, m)) + 2.0 * np.sqrt(m) * np.eye(m)
    Nr = nblk * p
    buf = Buffers(ex, dtype, W, Nr, np.random.default_rng(m + 1).permutation(Nr).astype(np.int32),
                  np.zeros(Nr, np.int32), done=I_SENT)
    before = buf.state()
    fused, mirror = buf.select(p, p - 1, nblk, 2)
    assert fused is False
    assert mirror is None if p > 1 else mirror[0] == -1  # the pinned mirror was never written
    st = buf.state()
    for n, v in st.items():
        assert v.tobytes() == before[n].tobytes(), n
    assert (st["inv_t"] == F_SENT).all() and (st["scores"] == F_SENT).all() and (st["valid"] == I_SENT).all()
    assert (st["seq"] == I_SENT).all() and (st["rec"] == B_SENT).all() and (st["out"] == B_SENT).all()
    assert st["done"][0] == I_SENT
