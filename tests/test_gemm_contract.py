"""Device::gemm / gemm_batch against their contract (csrc/include/gj/device.hpp, GemmExtra), on both
executors and, on the GPU, through every kernel family of csrc/kernels/gemm.hip.

Reference.  `_reference` computes the contract in numpy longdouble from the operands as stored in
the kernel's type: the expected C, which elements of C and of -C^T the call may write, and
S = |C_in after masks| + |A| |B|.

Embedding.  Every operand is an interior view of a larger parent tensor, as the engine's panels are:
a non-zero row and column origin, a leading dimension wider than the view and at least one tile of
margin (128 rows, 256 columns) on every side, so that a stray access of a wrong kernel lands in the
test's own memory.  Input parents hold NaN outside the view, output parents a sentinel.  Whatever the
contract says is not read holds NaN as well: C in its zero columns / zero row blocks, the skipped
columns of C and B, all of C when c_in or Store replaces it, the rows of A a row-block selection
leaves out; rows k >= K are the NaN margin.  A finite result proves none of it was read.  After the
call every byte of the C and -C^T parents outside the writable set, and every byte of the inputs,
is compared with a copy taken before.

Bound.  Componentwise |got - ref| <= gamma(K + 1) S, gamma(n) = n u / (1 - n u), u = 2^-53 (fp64) or
2^-24 (fp32).  Derived, not measured: every kernel here is a chain of K fused multiply-adds per
element starting from the accumulator input (one rounding per term and no flushing on the matrix
cores, in any order of the terms), which gives gamma(K) S; the host executor rounds each product
and each addition in double, at most K + 1 roundings per term.  The extra u S also covers the
longdouble reference's own error, at most K 2^-64 S = K 2^-11 u S.  Operands are uniform in [-1, 1)
or graded (row i of A scaled by 2^((7 i) % 61 - 30), column j of B by 2^((5 j) % 41 - 20), C_in by
both), where an absolute tolerance would hide whole rows.  `-s` prints, per kernel family, the
largest |got - ref| / (u S) seen.

Every GPU case asserts native.last_gemm_kernel(), so a dispatch fallback cannot turn a case into a
test of another kernel unnoticed; the host executor runs each distinct contract case once.
"""
import functools

import numpy as np
import pytest
import torch

from mpi_jordan_crazy_acceleration_amd import ops

LD = np.longdouble
F64, F32 = torch.float64, torch.float32
_NP = {F64: np.float64, F32: np.float32}
_U = {F64: LD(2) ** -53, F32: LD(2) ** -24}
_BITS = {F64: torch.int64, F32: torch.int32}
_TAG = {F64: "f64", F32: "f32"}
RM, CM = 128, 256  # margins: one tile of the tallest / widest kernel
SENT = -777.25     # exact in both types
K_RECORDS = 0x7FFFFFF0  # extent of every buffer resource in gemm.hip
K_MAX_BATCH = 4         # gemm.hip kMaxBatch: products per batched launch
RATIOS = {}


def gamma(n, u):
    return n * u / (1 - n * u)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RATIOS:
        print("\nlargest |got - ref| / (u S) per kernel family (the bound is gamma(K + 1) / u ~ K + 1):")
        for fam in sorted(RATIOS):
            r, k = RATIOS[fam]
            print(f"  {fam:24s} {r:8.3f}   (K = {k})")


# ------------------------------------------------------------------ operands and reference
@functools.lru_cache(maxsize=24)
def _operands(dtype, flavour, Mp, N, K):
    rng = np.random.default_rng([17, Mp, N, K, flavour == "graded"])
    A = rng.uniform(-1, 1, (Mp, K))
    B = rng.uniform(-1, 1, (K, N))
    Cin = rng.uniform(-1, 1, (Mp, N))
    if flavour == "graded":
        ra = np.ldexp(1.0, (np.arange(Mp) * 7) % 61 - 30)[:, None]
        cb = np.ldexp(1.0, (np.arange(N) * 5) % 41 - 20)[None, :]
        A, B, Cin = A * ra, B * cb, Cin * ra * cb
    out = tuple(np.ascontiguousarray(x.astype(_NP[dtype])) for x in (A, B, Cin))
    for x in out:
        x.setflags(write=False)
    return out


def _rows(c):
    """physical row of each of the product's M rows"""
    if c.get("rsel"):
        blocks, m = c["rsel"]
        return np.concatenate([np.arange(b * m, (b + 1) * m) for b in sorted(blocks)])
    return np.arange(c["M"])


@functools.lru_cache(maxsize=64)
def _product(dtype, flavour, Mp, N, K, rsel_key):
    A, B, _ = _operands(dtype, flavour, Mp, N, K)
    rows = _rows({"rsel": rsel_key, "M": Mp})
    Al, Bl = A[rows].astype(LD), B.astype(LD)
    return Al @ Bl, np.abs(Al) @ np.abs(Bl)


def _owned(owner):
    if owner is None or owner[2] is None:
        return True
    p, k, g = owner
    return g >= 0 and g % p == k


def _reference(c, A, B, Cin, rows):
    """The GemmExtra contract: (expected C on the product's rows [M x N], S, writable columns of C,
    writable columns of -C^T or None, whether the owner predicate lets the call run)."""
    M, N = len(rows), B.shape[1]
    P, absP = _product(c["dtype"], c["flavour"], A.shape[0], N, c["K"], _rsel_key(c))
    cols = np.arange(N)
    s0, s1 = c.get("skip", (0, 0))
    wcol = ~((cols >= s0) & (cols < s1))
    acc = Cin[rows].astype(LD)
    if c["op"] == "store":
        acc[:] = 0
    else:
        z0, z1 = c.get("zc", (0, 0))
        acc[:, z0:z1] = 0
        zr, zh = c.get("zr", ((), 0))
        for r in zr:  # physical rows, also under a row-block selection
            acc[(rows >= r) & (rows < r + zh)] = 0
    tcol = None
    if c.get("tneg") is not None:
        tcol = wcol & (cols < (c["tneg"] or N))
    return acc + P, np.abs(acc) + absP, wcol, tcol, _owned(c.get("owner"))


def _rsel_key(c):
    return (tuple(c["rsel"][0]), c["rsel"][1]) if c.get("rsel") else None


# ------------------------------------------------------------------ embedding
def _embed(arr, dev, fill, pad, origin=None):
    ro, co, ldx = origin or (RM, CM, 0)
    h, w = arr.shape
    ld = -(-(co + w + CM) // 4) * 4 + pad + ldx
    parent = torch.full((ro + h + RM, ld), fill, dtype=torch.from_numpy(arr[:1, :1]).dtype, device=dev)
    view = parent[ro:ro + h, co:co + w]
    view.copy_(torch.from_numpy(arr))
    return parent, view


def _bits(t):
    return t.view(_BITS[t.dtype])


def _changed_outside(parent, before, view_origin, allowed_rows=None, allowed_cols=None):
    """number of elements of `parent` whose bytes changed outside view[allowed_rows x allowed_cols]"""
    changed = _bits(parent) != _bits(before)
    if allowed_rows is not None and len(allowed_rows) and len(allowed_cols):
        ro, co = view_origin
        r = torch.as_tensor(allowed_rows + ro, device=parent.device).unsqueeze(1)
        cc = torch.as_tensor(allowed_cols + co, device=parent.device).unsqueeze(0)
        changed[r, cc] = False
    return int(changed.sum().item())


def _dev(ex):
    return "cuda" if ex == "gpu" else "cpu"


_SETTERS = {"variant": ("set_gemm_variant", "auto"), "lat_kernel": ("set_lat_kernel", -1),
            "glds_tile": ("set_glds_tile", 0), "glds_build": ("set_glds_build", 0),
            "glds_peel": ("set_glds_peel", True), "glds_covl": ("set_glds_covl", True),
            "lat_glds": ("set_lat_glds", False)}


class _forced:
    """the process-wide kernel choices of a case, restored on exit"""

    def __init__(self, native, setters):
        self.native, self.setters = native, setters

    def __enter__(self):
        for k, v in self.setters.items():
            getattr(self.native, _SETTERS[k][0])(v)

    def __exit__(self, *exc):
        for k in self.setters:
            getattr(self.native, _SETTERS[k][0])(_SETTERS[k][1])


def _prepare(c, ex):
    """the stored operands of case c (poisoned where the contract says nothing is read), embedded"""
    dtype, dev = c["dtype"], _dev(ex)
    M, N, K = c["M"], c["N"], c["K"]
    rows = _rows(c)
    Mp = c.get("Mp", M)
    A, B, Cin = _operands(dtype, c["flavour"], Mp, N, K)
    s0, s1 = c.get("skip", (0, 0))
    nan = np.nan
    As = A.copy()
    if c.get("rsel"):
        keep = np.zeros(Mp, bool)
        keep[rows] = True
        As[~keep] = nan
    Bs = B.copy()
    Bs[:, s0:s1] = nan
    Ci = Cin.copy()  # the accumulator's input as stored: NaN under every mask
    z0, z1 = c.get("zc", (0, 0))
    Ci[:, z0:z1] = nan
    Ci[:, s0:s1] = nan
    zr, zh = c.get("zr", ((), 0))
    for r in zr:
        Ci[max(r, 0):r + zh] = nan
    org = c.get("origin", {})
    t = {}
    t["Ap"], t["A"] = _embed(As.T.copy() if c["kmajor"] else As, dev, nan, 4, org.get("A"))
    t["Bp"], t["B"] = _embed(Bs, dev, nan, 8, org.get("B"))
    if c["op"] == "store" or c.get("cin"):
        Cs = np.full_like(Cin, nan)
    else:
        Cs = Ci
    t["Cp"], t["C"] = _embed(Cs, dev, SENT, 12, org.get("C"))
    t["Cin"] = None
    if c.get("cin"):
        t["Cinp"], t["Cin"] = _embed(Ci, dev, SENT, 16, org.get("Cin"))
    t["T"] = None
    if c.get("tneg") is not None:
        tc = c["tneg"] or N
        t["Tp"], t["T"] = _embed(np.full((tc, Mp), SENT, _NP[dtype]), dev, SENT, 20, org.get("T"))
    t["phys"] = None
    if c.get("owner") is not None and c["owner"][2] is not None:
        t["phys"] = torch.tensor([c["owner"][2], 12345], dtype=torch.int32, device=dev)
    t["rows"], t["clean"] = rows, (A, B, Cin)
    return t


def _gemm_kwargs(c, t):
    kw = dict(op=c["op"], a_kmajor=c["kmajor"], c_in=t["Cin"], tneg=t["T"])
    if "zc" in c:
        kw["zero_cols"] = c["zc"]
    if "zr" in c:
        kw["zero_rows"], kw["zero_row_height"] = c["zr"]
    if "skip" in c:
        kw["skip_cols"] = c["skip"]
    if c.get("rsel"):
        kw["row_blocks"], kw["row_block_m"] = c["rsel"]
    if c.get("owner") is not None:
        kw["owner"] = (t["phys"], c["owner"][0], c["owner"][1])
    kw.update(c.get("kw", {}))
    return kw


def _check(c, t, fam):
    """bound on what may be written, identity of everything else"""
    dtype = c["dtype"]
    A, B, Cin = t["clean"]
    rows = t["rows"]
    expC, S, wcol, tcol, active = _reference(c, A, B, Cin, rows)
    u = _U[dtype]
    bound = gamma(c["K"] + 1, u) * S
    org = c.get("origin", {})
    co = (org.get("C") or (RM, CM, 0))[:2]
    wc = np.nonzero(wcol)[0]
    n_bad = _changed_outside(t["Cp"], t["Cp0"], co, rows if active else None, wc)
    assert n_bad == 0, f"{n_bad} elements of C's parent changed outside the writable set"
    if t["T"] is not None:
        to = (org.get("T") or (RM, CM, 0))[:2]
        tcs = np.nonzero(tcol)[0]
        n_bad = _changed_outside(t["Tp"], t["Tp0"], to, tcs if active else None, rows)
        assert n_bad == 0, f"{n_bad} elements of the -C^T parent changed outside the writable set"
    for name in ("Ap", "Bp", "Cinp"):
        if name in t:
            assert torch.equal(_bits(t[name]), _bits(t[name + "0"])), f"input parent {name} changed"
    if t["phys"] is not None:
        assert t["phys"].cpu().tolist() == [c["owner"][2], 12345]
    if not active:
        return
    rt = torch.as_tensor(rows, device=t["C"].device)
    got = t["C"][rt].cpu().numpy()
    err = np.abs(got.astype(LD) - expC)
    ratio = float((err[:, wc] / (u * S[:, wc])).max())
    print(f"{c['id']}: {fam}  max |got - ref| / (u S) = {ratio:.3f}  (gamma(K + 1) / u = "
          f"{float(gamma(c['K'] + 1, u) / u):.3f})")
    if np.isfinite(ratio) and ratio > RATIOS.get(fam, (-1, 0))[0]:
        RATIOS[fam] = (ratio, c["K"])
    ok = err[:, wc] <= bound[:, wc]  # (False for a NaN)
    assert ok.all(), (f"{int((~ok).sum())} elements of C beyond gamma(K + 1) S, worst ratio to the bound "
                      f"{float(np.nanmax(err[:, wc] / bound[:, wc])):.3g}, non-finite {int((~np.isfinite(got[:, wc])).sum())}")
    if t["T"] is not None:
        gotT = t["T"][:, rt].cpu().numpy()
        tcs = np.nonzero(tcol)[0]
        assert np.array_equal(gotT[tcs], -got[:, tcs].T), "-C^T is not the negated transpose of the stored C"


def _run(c, ex, native):
    t = _prepare(c, ex)
    for name in ("Ap", "Bp", "Cp", "Cinp", "Tp"):
        if name in t:
            t[name + "0"] = t[name].clone()
    kw = _gemm_kwargs(c, t)
    with _forced(native, c.get("setters", {}) if ex == "gpu" else {}):
        ops.gemm(t["A"], t["B"], t["C"], **kw)
        fam = native.last_gemm_kernel()
    assert fam == (c["fam"] if ex == "gpu" else "host"), f"ran {fam}"
    _check(c, t, fam)


# ------------------------------------------------------------------ the cases
REG_K, G64_K, G32_K, LAT_K = (5, 16, 17, 60), (5, 16, 24, 43, 136), (5, 32, 48, 83), (5, 32, 64, 70, 130)
SHAPES = ((332, 540), (130, 70))
ZR4 = ((0, 120, 180, 300), 60)                        # spans the 128-row tile edge; the last block passes M
ZR8 = ((0, 40, 80, 120, 140, 180, 240, 320), 20)      # kMaxZeroRows blocks
ZR_SMALL = ((0, 120), 60)


def _fam(name, dtype, fam, setters=None, kw=None, Ks=REG_K, kx=60, kmajor=True, shapes=SHAPES, skip=(128, 384)):
    return dict(name=name, dtype=dtype, fam=fam, setters=setters or {}, kw=kw or {}, Ks=Ks, kx=kx, kmajor=kmajor,
                shapes=shapes, skip=skip)


LATENCY = {"latency": True}
FAMILIES = [
    _fam("small", F64, "small", {"lat_kernel": 0}, LATENCY),
    _fam("lat64-reg", F64, "lat64", {"lat_kernel": -1}, {"latency": True, "lat_reg": True}, LAT_K, 70),
    _fam("lat64-set", F64, "lat64", {"lat_kernel": 1}, LATENCY, LAT_K, 70),
    _fam("narrow", F64, "narrow", {"variant": "narrow"}),
    _fam("big", F64, "big", {"variant": "big"}),
    _fam("bigpf", F64, "bigpf", {"variant": "bigpf"}),
    _fam("squarepf", F64, "squarepf", {"variant": "squarepf"}),
    _fam("g64-t64-b23", F64, "glds64:t64:b23:peel", {"glds_tile": 64}, {"glds_build": 23}, G64_K, 43),
    _fam("g64-t64-b25", F64, "glds64:t64:b25:peel", {}, {"dense": True}, G64_K, 43),
    _fam("g64-t64-b33", F64, "glds64:t64:b33:peel", {}, {"glds_tile": 64, "glds_build": 33}, G64_K, 43),
    _fam("g64-t64-b23-nopeel", F64, "glds64:t64:b23", {"glds_peel": False}, {"glds_build": 23}, G64_K, 43),
    _fam("g64-t128-b23", F64, "glds64:t128:b23:peel", {}, {"glds_tile": 128, "glds_build": 23}, G64_K, 43),
    _fam("g64-t128-b33", F64, "glds64:t128:b33:peel", {"glds_tile": 128}, {"glds_build": 33}, G64_K, 43),
    _fam("g64-t128-b32", F64, "glds64:t128:b32:peel", {}, {"glds_build": 32}, G64_K, 43),
    _fam("lat-wide", F64, "glds64:t128:b23:peel", {}, {"latency": True, "lat_wide": True}, G64_K, 43,
         shapes=((1156, 140),), skip=(0, 128)),
    _fam("small32", F32, "small", {}, LATENCY),
    _fam("narrow32", F32, "narrow", {"variant": "narrow"}),
    _fam("squarepf32", F32, "squarepf", {"variant": "squarepf"}),
    # (130 x 70 is no multiple of 4: the fp32 LDS-DMA kernel cannot take it, see the fallbacks)
    _fam("g32-t128", F32, "glds32:t128", {"variant": "glds"}, {"glds_tile": 64}, G32_K, 83,
         shapes=((332, 540), (132, 68))),
    _fam("g32-t256", F32, "glds32:t256", {"variant": "glds"}, {}, G32_K, 83, shapes=((332, 540), (132, 68)),
         skip=(256, 512)),
    _fam("rowmajor-auto", F64, "narrow", {}, {}, kmajor=False),
    _fam("rowmajor-narrow", F64, "narrow", {"variant": "narrow"}, {}, kmajor=False),
    _fam("rowmajor-auto32", F32, "narrow", {}, {}, kmajor=False),
    _fam("rowmajor-narrow32", F32, "narrow", {"variant": "narrow"}, {}, kmajor=False),
]


def _extras(f):
    """each GemmExtra field alone, then the combinations the engine issues (engine.cpp: MAIN's chunk
    update, the chain's column update, the look-ahead update, the chunk pass, the piece batch)"""
    sk = f["skip"]
    e = [("store", dict(op="store")),
         ("zc", dict(zc=(100, 230))),
         ("zr4", dict(zr=ZR4)),
         ("zr8", dict(zr=ZR8)),
         ("cin", dict(cin=True)),
         ("tneg", dict(tneg=0)),
         ("tneg-cols", dict(tneg=70)),
         ("skip", dict(skip=sk)),
         ("cnt3", dict(kw={"c_nt": 3})),
         ("cnt1", dict(kw={"c_nt": 1}, zc=(100, 230))),
         ("owner-nophys", dict(owner=(3, 1, None))),
         # MAIN's chunk update: the panel's block columns and pivot rows enter as 0, around the look-ahead cut
         ("main-chunk", dict(zc=(100, 230), zr=ZR8, skip=sk, kw={"c_nt": 3})),
         # the chunk pass: X row -> temp through C_in
         ("chunk-pass", dict(cin=True, zc=(100, 230), skip=sk)),
         ("cin-zr8", dict(cin=True, zr=ZR8, zc=(100, 230))),
         # look-ahead / column update: the next multiplier panel from the first columns
         ("lookahead", dict(tneg=70, zr=ZR4)),
         ("tneg-skip", dict(tneg=0, skip=sk)),
         # the host-free chain's predicated launches
         ("owner-true", dict(cin=True, owner=(3, 1, 7))),
         ("owner-false", dict(cin=True, owner=(3, 1, 6))),
         ("owner-none", dict(cin=True, owner=(3, 1, -1))),
         ("owner-false-tneg", dict(tneg=0, owner=(2, 0, 5)))]
    if f["fam"].startswith("glds"):
        e.append(("covl-off", dict(setters={"glds_covl": False}, zc=(100, 230), zr=ZR4)))
    if f["name"] == "g64-t128-b23":  # MAIN's chunk update under a CU reservation: the dense build
        e.append(("main-chunk-dense", dict(zc=(100, 230), zr=ZR8, skip=sk, kw={"c_nt": 3, "dense": True, "glds_build": 0,
                                                                                 "glds_tile": 0},
                                           fam="glds64:t64:b25:peel")))
    return e


SMALL_EXTRAS = [("mix", dict(zc=(20, 50), zr=ZR_SMALL, tneg=30)),
                ("cin-zc", dict(cin=True, zc=(20, 50), zr=ZR_SMALL)),
                ("store", dict(op="store"))]


def _expected(f, x):
    """the kernel the dispatcher picks for family f under extras x (launch<> in gemm.hip)"""
    fam, setters = x.get("fam", f["fam"]), dict(f["setters"])
    if x.get("cin") and not f["kw"].get("latency"):
        # C_in: the LDS-DMA kernels under "auto" only, else the narrow register tile
        if fam.startswith("glds32"):
            setters["variant"] = "auto"
        elif setters.get("variant", "auto") != "auto":
            fam = "narrow"
    if x.get("tneg") is not None and fam.startswith("glds32"):
        fam = "squarepf"  # the fp32 LDS-DMA kernel has no -C^T epilogue
    return fam, setters


def _case(f, tag, M, N, K, flavour, x):
    fam, setters = _expected(f, x)
    setters.update(x.get("setters", {}))
    c = dict(id=f"{f['name']}-{M}x{N}x{K}-{flavour}-{tag}", dtype=f["dtype"], kmajor=f["kmajor"], M=M, N=N, K=K,
             flavour=flavour, op=x.get("op", "acc"), fam=fam, setters=setters, kw={**f["kw"], **x.get("kw", {})})
    for k in ("zc", "zr", "cin", "tneg", "skip", "owner", "rsel", "Mp", "origin"):
        if k in x:
            c[k] = x[k]
    return c


def _family_cases():
    out = []
    for f in FAMILIES:
        (M, N), small = f["shapes"][0], f["shapes"][-1]
        for i, K in enumerate(f["Ks"]):  # every phase of the K loop, both shapes
            out.append(_case(f, "acc", M, N, K, "uniform" if i % 2 == 0 else "graded", {}))
            if small != (M, N):
                out.append(_case(f, "acc", small[0], small[1], K, "graded" if i % 2 == 0 else "uniform", {}))
        for i, (tag, x) in enumerate(_extras(f)):
            if N < 256 and "skip" in x and x.get("zc"):
                x = {**x, "zc": (20, 50)}
            out.append(_case(f, tag, M, N, f["kx"], "graded" if i % 2 == 0 else "uniform", x))
        if small != (M, N):
            for tag, x in SMALL_EXTRAS:
                out.append(_case(f, tag, small[0], small[1], f["kx"], "graded", x))
    return out


# Row-block selections: blocks in words 0, 1 and 7 of the bit map; the physical height is what the
# highest block needs.  Zero rows are physical: one block inside a selected row block, one inside an
# unselected one (whose logical namesake is selected), one running over the end of a selected block.
R64, R128 = ([0, 63, 64, 130, 511], 64), ([1, 64, 255], 128)
ZR_R64, ZR_R128 = ((63 * 64 + 10, 70, 130 * 64 + 50), 30), ((128 + 100, 64 * 128 + 5, 50), 30)


def _rsel_cases():
    f64 = lambda fam, setters=None, kw=None: _fam("rsel", F64, fam, setters, kw)  # noqa: E731
    f32 = lambda fam, setters=None, kw=None: _fam("rsel32", F32, fam, setters, kw)  # noqa: E731
    big64, big128 = dict(rsel=R64, Mp=512 * 64), dict(rsel=R128, Mp=256 * 128)
    rows = [
        # the chain's column update: rsel + tneg + latency (+ lat_reg / lat_wide)
        (f64("small", {"lat_kernel": 0}, LATENCY), "r64-chain", 96, 60, dict(big64, tneg=0, zr=ZR_R64)),
        (f64("small", {"lat_kernel": -1}, {"latency": True, "lat_reg": True}), "r64-chain-latreg", 96, 60,
         dict(big64, tneg=0)),
        (f64("small"), "r64-deferred", 96, 17, dict(big64, tneg=40, zr=ZR_R64, cin=True)),
        (f64("small", {"lat_kernel": 0}, LATENCY), "r128-chain", 96, 60, dict(big128, tneg=0, zr=ZR_R128)),
        (f64("glds64:t128:b23:peel", {}, {"latency": True, "lat_wide": True}), "r128-chain-latwide", 96, 43,
         dict(big128, tneg=0, zr=ZR_R128)),
        (f64("glds64:t128:b23:peel"), "r128-deferred", 96, 43, dict(big128, tneg=40, zr=ZR_R128)),
        (f64("glds64:t64:b33:peel", {}, {"glds_tile": 64}), "r128-cin", 96, 24, dict(big128, cin=True, zc=(30, 70))),
        (f64("narrow", {"variant": "narrow"}), "r128-narrow", 96, 17, dict(big128, zr=ZR_R128)),
        # rsel x skip (the physical height of block 130 / 64)
        (f64("small"), "r64-skip", 300, 17, dict(rsel=(R64[0][:4], 64), Mp=131 * 64, skip=(128, 256), tneg=0,
                                                   zr=ZR_R64)),
        (f64("glds64:t128:b23:peel"), "r128-skip", 300, 43, dict(rsel=(R128[0][:2], 128), Mp=65 * 128, skip=(128, 256),
                                                                   tneg=0, zr=ZR_R128)),
        (f32("small", {}, LATENCY), "r64-chain", 96, 60, dict(big64, tneg=0, zr=ZR_R64)),
        (f32("glds32:t256"), "r128-deferred", 96, 83, dict(big128, zr=ZR_R128)),
        (f32("glds32:t128", {}, {"glds_tile": 64}), "r128-cin", 96, 48, dict(big128, cin=True, zc=(30, 70))),
        (f32("narrow"), "r128-tneg", 96, 17, dict(big128, tneg=40, zr=ZR_R128)),
        (f32("small", {}, LATENCY), "r128-chain", 96, 17, dict(big128, tneg=0)),
        (f32("glds32:t128"), "r128-skip", 300, 83, dict(rsel=(R128[0][:2], 128), Mp=65 * 128, skip=(128, 256))),
    ]
    out = []
    for i, (f, tag, N, K, x) in enumerate(rows):
        M = len(x["rsel"][0]) * x["rsel"][1]
        x = dict(x, fam=f["fam"])
        c = _case(f, tag, M, N, K, "graded" if i % 2 == 0 else "uniform", x)
        c["fam"] = f["fam"]  # (spelled out per row above: no rule applied)
        c["setters"] = {**f["setters"]}
        out.append(c)
    return out


# Dispatch fallbacks of glds_ok / glds32_ok / launch_glds32, asked for with the "glds" variant: fp64
# falls to bigpf, fp32 to squarepf; under "auto" a shallow product falls to the narrow tile.
def _fallback_cases():
    g64 = _fam("fallback", F64, "bigpf", {"variant": "glds"}, Ks=(43,), kx=43)
    g32 = _fam("fallback32", F32, "squarepf", {"variant": "glds"}, Ks=(83,), kx=83)
    odd = (RM, CM + 1, 0)   # the view begins at an odd element: not 16-byte aligned
    oddld = (RM, CM, 1)     # an odd leading dimension
    out = []
    for f in (g64, g32):
        K = f["kx"]
        out += [_case(f, "A-origin-odd", 332, 540, K, "uniform", dict(origin={"A": odd}, zc=(100, 230))),
                _case(f, "B-origin-odd", 332, 540, K, "graded", dict(origin={"B": odd}, zr=ZR4)),
                _case(f, "lda-odd", 332, 540, K, "graded", dict(origin={"A": oddld}, tneg=70)),
                _case(f, "ldb-odd", 332, 540, K, "uniform", dict(origin={"B": oddld}, skip=(128, 384)))]
    out += [_case(g64, "M-odd", 331, 540, 43, "graded", dict(zr=ZR4)),
            _case(g64, "N-odd", 332, 541, 43, "uniform", dict(zc=(100, 230))),
            _case(g32, "M-mod4", 330, 540, 83, "graded", dict(zr=ZR4)),
            _case(g32, "N-mod4", 332, 542, 83, "uniform", dict(zc=(100, 230))),
            _case(g32, "130x70", 130, 70, 83, "graded", {}),
            _case(g32, "lda-mod4", 332, 540, 83, "uniform", dict(origin={"A": (RM, CM, 2)})),
            # C and C_in need no alignment: still the LDS-DMA kernels
            _case(_fam("aligned-c-odd", F64, "glds64:t128:b23:peel", Ks=(43,), kx=43), "C-origin-odd", 332, 540, 43,
                  "graded", dict(origin={"C": odd, "Cin": (RM, CM + 3, 1), "T": odd}, cin=True, tneg=70)),
            _case(_fam("auto-odd", F64, "narrow", Ks=(43,), kx=43), "A-origin-odd", 332, 540, 43, "graded",
                  dict(origin={"A": odd})),
            # whole-tile skip: the 256-wide fp32 tile takes (256, 512) but not (128, 384)
            _case(_fam("t256-skip", F32, "glds32:t128", {"variant": "glds"}, Ks=(83,), kx=83), "skip-128-384", 332, 540,
                  83, "graded", dict(skip=(128, 384), zc=(100, 230))),
            _case(_fam("t256-skip", F32, "glds32:t256", {"variant": "glds"}, Ks=(83,), kx=83), "skip-256-512", 332, 540,
                  83, "graded", dict(skip=(256, 512), zc=(100, 230)))]
    return out


GPU_CASES = _family_cases() + _rsel_cases() + _fallback_cases()
assert len({c["id"] for c in GPU_CASES}) == len(GPU_CASES)


def _contract_key(c):
    """what the host executor sees of a case: everything but the kernel choice"""
    return repr([(k, c.get(k)) for k in ("dtype", "kmajor", "M", "N", "K", "flavour", "op", "zc", "zr", "cin", "tneg",
                                          "skip", "owner", "rsel", "Mp", "origin")])


def _host_cases():
    seen, out = set(), []
    for c in GPU_CASES:
        k = _contract_key(c)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


HOST_CASES = _host_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("c", GPU_CASES, ids=[c["id"] for c in GPU_CASES])
def test_gemm_contract_gpu(c, native):
    _run(c, "gpu", native)


@pytest.mark.parametrize("c", HOST_CASES, ids=[c["id"] for c in HOST_CASES])
def test_gemm_contract_host(c, native):
    _run(c, "cpu", native)


def test_every_family_and_field_is_covered():
    """every kernel family the dispatcher can name has a case asserting it, and every GemmExtra field
    is set by at least one case"""
    fams = {c["fam"] for c in GPU_CASES} | {"batch:small", "batch:lat"}  # (the batch tests below)
    want = {"small", "narrow", "big", "bigpf", "squarepf", "lat64", "glds64:t64:b23:peel", "glds64:t64:b25:peel",
            "glds64:t64:b33:peel", "glds64:t64:b23", "glds64:t128:b23:peel", "glds64:t128:b33:peel",
            "glds64:t128:b32:peel", "glds32:t128", "glds32:t256", "batch:small", "batch:lat"}
    assert want <= fams, want - fams
    for field in ("zc", "zr", "cin", "tneg", "skip", "owner", "rsel"):
        assert any(field in c for c in GPU_CASES), field
    for field in ("latency", "lat_wide", "lat_reg", "glds_build", "glds_tile", "c_nt", "dense"):
        assert any(c["kw"].get(field) for c in GPU_CASES), field
    assert any(len(c["zr"][0]) == 8 for c in GPU_CASES if "zr" in c)
    assert any(max(c["rsel"][0]) >= 7 * 64 for c in GPU_CASES if "rsel" in c)


# ------------------------------------------------------------------ gemm_batch
def _batch_products(dtype, count, lat, false_at):
    """`count` K-major products of different K, Store and Acc mixed; product `false_at` (if any)
    carries an owner predicate that is false, the one after it a true one"""
    ps = []
    shapes = [(130, 70), (64, 32), (37, 100), (200, 33), (128, 64)]
    Ks = LAT_K if lat else REG_K
    for i in range(count):
        M, N = shapes[i % len(shapes)]
        c = dict(id=f"p{i}", dtype=dtype, kmajor=True, M=M + i, N=N, K=Ks[i % len(Ks)] + (i // len(Ks)),
                 flavour="graded" if i % 2 else "uniform", op="store" if i % 3 == 1 else "acc", kw={})
        if i == false_at:
            c["owner"] = (3, 1, 5)
        elif false_at is not None and i == false_at + 1:
            c["owner"] = (3, 1, 4)
        ps.append(c)
    return ps


def _run_batch(dtype, count, lat, false_at, ex, native):
    cases = _batch_products(dtype, count, lat, false_at)
    ts, items = [], []
    for c in cases:
        t = _prepare(c, ex)
        for name in ("Ap", "Bp", "Cp"):
            t[name + "0"] = t[name].clone()
        ts.append(t)
        extra = {"lat_reg": lat}
        if c.get("owner") is not None:
            extra["owner"] = (t["phys"], c["owner"][0], c["owner"][1])
        items.append((c["op"], t["A"], t["B"], t["C"], extra))
    with _forced(native, {"lat_kernel": -1} if ex == "gpu" else {}):
        ops.gemm_batch(items)
        fam = native.last_gemm_kernel()
    assert fam == (("batch:lat" if lat else "batch:small") if ex == "gpu" else "host"), fam
    for c, t in zip(cases, ts):
        _check(c, t, fam)


BATCH = [(F64, False), (F64, True), (F32, False)]
BATCH_COUNTS = [(1, None), (K_MAX_BATCH, None), (7, 0), (7, 5), (2 * K_MAX_BATCH + 1, 8), (9, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("count,false_at", BATCH_COUNTS)
@pytest.mark.parametrize("dtype,lat", BATCH)
def test_gemm_batch_contract_gpu(dtype, lat, count, false_at, native):
    """1, 7 and 9 products cross kMaxBatch = 4 once and twice; an owner predicate is per product"""
    _run_batch(dtype, count, lat, false_at, "gpu", native)


@pytest.mark.parametrize("count,false_at", BATCH_COUNTS)
@pytest.mark.parametrize("dtype", [F64, F32])
def test_gemm_batch_contract_host(dtype, count, false_at, native):
    _run_batch(dtype, count, False, false_at, "cpu", native)


# ------------------------------------------------------------------ non-finite operands
NONFINITE = [("host", "cpu", F64, {}, {}), ("host", "cpu", F32, {}, {}),
             ("small", "gpu", F64, {"lat_kernel": 0}, LATENCY), ("lat64", "gpu", F64, {"lat_kernel": 1}, LATENCY),
             ("narrow", "gpu", F64, {"variant": "narrow"}, {}), ("bigpf", "gpu", F64, {"variant": "bigpf"}, {}),
             ("glds64:t64:b33:peel", "gpu", F64, {}, {"glds_tile": 64}), ("glds64:t128:b23:peel", "gpu", F64, {}, {}),
             ("small", "gpu", F32, {}, LATENCY), ("narrow", "gpu", F32, {"variant": "narrow"}, {}),
             ("squarepf", "gpu", F32, {"variant": "squarepf"}, {}),
             ("glds32:t128", "gpu", F32, {"variant": "glds"}, {"glds_tile": 64}),
             ("glds32:t256", "gpu", F32, {"variant": "glds"}, {})]


@pytest.mark.parametrize("fam,ex,dtype,setters,kw", [
    pytest.param(*n, marks=[pytest.mark.gpu] if n[1] == "gpu" else [], id=f"{n[0]}-{_TAG[n[2]]}") for n in NONFINITE])
def test_gemm_nonfinite_reaches_every_chain(fam, ex, dtype, setters, kw, native):
    """Device::gemm's rule, the same on both executors: a NaN / Inf of B inside the product reaches
    every element of C whose sum it is a term of, also through a zero factor of A (0 * NaN = 0 * Inf
    = NaN on the matrix cores; the host executor must not skip zero multipliers); every other
    element stays finite.  A NaN under a mask (a skipped column of B) reaches nothing."""
    M, N, K, k0, jn, ji = 132, 520, 36, 9, 3, 517
    A, B, Cin = (x.copy() for x in _operands(dtype, "uniform", M, N, K))
    A[:70, k0] = 0          # a zero factor for the first rows, across a 64-row tile edge
    B[k0, jn] = np.nan
    B[k0, ji] = np.inf
    B[:, 256:512] = np.nan  # skipped (whole tiles of every kernel)
    dev = _dev(ex)
    At, Bt, Ct = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (A.T, B, Cin))
    with _forced(native, setters if ex == "gpu" else {}):
        ops.gemm(At, Bt, Ct, op="acc", a_kmajor=True, skip_cols=(256, 512), **kw)
        assert native.last_gemm_kernel() == fam
    got = Ct.cpu().numpy()
    bad = ~np.isfinite(got)
    want = np.zeros((M, N), bool)
    want[:, jn] = True
    want[:, ji] = True
    assert np.array_equal(bad, want), (np.argwhere(bad != want)[:8].tolist(), int((bad != want).sum()))
    assert np.isnan(got[:, jn]).all() and np.isnan(got[:70, ji]).all() and np.isinf(got[70:, ji]).all()
    assert np.array_equal(got[:, 256:512], Cin[:, 256:512])


# ------------------------------------------------------------------ leading dimensions and 32-bit tile offsets
# A tile addresses its operand rows with 32-bit byte offsets below K_RECORDS: the largest offset is
# ((rows - 1) ld + cols) elements (gemm.hip check_cfg).  One-row views need no memory for the rows
# that a huge ld would put 2 GiB apart; M = 1 or K = 1 keeps every other row masked.
def _ld_limit(rows, cols, es):
    return (K_RECORDS // es - cols) // (rows - 1)


LD_TILES = {"small": (64, 32, 16), "narrow": (128, 64, 8)}  # BM, BN, BK


def _one_row(base, n, ld):
    return base.as_strided((1, n), (ld, 1))


LD_CASES = ([(f, d, w) for f in ("small", "narrow") for d in (F64, F32) for w in ("C", "Cin", "A", "B", "A-rowmajor")] +
            [("batch:small", d, w) for d in (F64, F32) for w in ("C", "A", "B")] +
            # what the LDS-DMA kernel's own check refuses falls to the narrow tile, which checks again
            [("auto", F64, "C"), ("auto", F64, "Cin")])


@pytest.mark.gpu
@pytest.mark.parametrize("fam,dtype,which", LD_CASES, ids=[f"{f}-{_TAG[d]}-{w}" for f, d, w in LD_CASES])
def test_gemm_leading_dimension_limit(fam, dtype, which, native):
    """the largest leading dimension a kernel's tile can address gives the reference's result, one
    more raises BadArgs (it used to mask the rows away: zeros loaded, stores dropped, no error)"""
    batch, auto = fam == "batch:small", fam == "auto"
    tile = "narrow" if auto else "small" if batch else fam
    BM, BN, BK = LD_TILES[tile]
    es = 8 if dtype == F64 else 4
    M, N, K = (1, 40, 1) if which in ("A", "B") else (1, 40, 8)
    if which == "A":
        M = 24
    limit = {"C": _ld_limit(BM, BN, es), "Cin": _ld_limit(BM, BN, es), "A": _ld_limit(BK, BM, es),
             "B": _ld_limit(BK, BN, es), "A-rowmajor": _ld_limit(BM, BK, es)}[which]
    rng = np.random.default_rng(5)
    A = rng.uniform(-1, 1, (M, K)).astype(_NP[dtype])
    B = rng.uniform(-1, 1, (K, N)).astype(_NP[dtype])
    Cin = rng.uniform(-1, 1, (M, N)).astype(_NP[dtype])
    ref = Cin.astype(LD) + A.astype(LD) @ B.astype(LD)
    S = np.abs(Cin).astype(LD) + np.abs(A).astype(LD) @ np.abs(B).astype(LD)
    setters = {} if auto else {"lat_kernel": 0} if tile == "small" else {"variant": "narrow"}
    kw = {"latency": True} if tile == "small" and not batch else {}
    for ld, ok in ((limit, True), (limit + 1, False)):
        rm = which == "A-rowmajor"
        At = torch.empty((M, K) if rm else (K, M), dtype=dtype).copy_(torch.from_numpy(A if rm else A.T)).cuda()
        Bt, Ct, Ci = torch.from_numpy(B).cuda(), torch.from_numpy(Cin).cuda(), None
        if which == "C":
            Ct = _one_row(Ct, N, ld)
        elif which == "Cin":
            Ci, Ct = _one_row(Ct.clone(), N, ld), torch.full_like(Ct, float("nan"))
        elif which == "A":
            At = _one_row(At, M, ld)
        elif which == "A-rowmajor":
            At = _one_row(At, K, ld)
        else:
            Bt = _one_row(Bt, N, ld)
        with _forced(native, setters):
            if batch:
                call = lambda: ops.gemm_batch([("acc", At, Bt, Ct)])  # noqa: E731
            else:
                call = lambda: ops.gemm(At, Bt, Ct, op="acc", a_kmajor=not rm, c_in=Ci, **kw)  # noqa: E731
            if ok:
                call()
                assert native.last_gemm_kernel() == (fam if not auto else "narrow")
                got = Ct.cpu().numpy().astype(LD)
                assert (np.abs(got - ref) <= gamma(K + 1, _U[dtype]) * S).all()
            else:
                with pytest.raises(native.GJError) as e:
                    call()
                assert e.value.status == 5, e.value.status  # Status::BadArgs
                assert torch.equal(Ct.cpu(), torch.from_numpy(Cin)) or which == "Cin"
