#!/usr/bin/env python3
"""gj.batched on one GPU (profiles/batched.md).

  e2e      gj.batched.factor of a random well-conditioned stack (nb, n, n) already on the GPU, and
           F.solve at k = 1 and k = 16: host clock around calls that end synchronised, a small stack
           warms every path up first, then the median of `--reps` runs.  The same stack through
           torch.linalg.inv and torch.linalg.solve on the same GPU in the stack's dtype, the same way.
           `outside`: the share of factor spent outside Device::block_inverse -- 1 - t(block_inverse on
           the packed panel of the whole stack, host clock, synchronised) / t(factor).
  kernels  Device::batch_pack, batch_unpack and batch_rhs (k = 16) alone by device events over `--reps`
           launches after a warm-up launch: microseconds and the compulsory traffic (every operand read or
           written once) in GB/s, set against a device-to-device copy that moves the same number of bytes
           (half read, half written), timed here by events too.

One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mpi_jordan_crazy_acceleration_amd as gj  # noqa: E402
from mpi_jordan_crazy_acceleration_amd import ops  # noqa: E402

_DT = {"fp64": torch.float64, "fp32": torch.float32}
SHAPES = [(16, 16384), (64, 8192), (128, 4096), (256, 1024), (1024, 64)]


def copy_us(nbytes, reps):
    """a device-to-device copy that moves nbytes in all (half read, half written), microseconds"""
    half = max(nbytes // 2 // 8, 1)
    src = torch.empty(half, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def wall_ms(f, reps):
    """median host-clock milliseconds of f(), synchronised; None where f fails (a comparison library's
    own limit must not end the run)"""
    try:
        f()
    except RuntimeError as e:
        print(json.dumps({"what": "failed", "error": str(e).splitlines()[0][:160]}), flush=True)
        torch.cuda.synchronize()
        return None
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def stack(n, nb, dt):
    g = torch.Generator(device="cuda").manual_seed(n * 131 + nb)
    A = torch.rand((nb, n, n), dtype=torch.float64, device="cuda", generator=g) * 2 - 1
    A += 2.0 * n ** 0.5 * torch.eye(n, dtype=torch.float64, device="cuda")
    return A.to(_DT[dt])


def e2e(n, nb, dt, reps):
    A = stack(n, nb, dt)
    out = {"what": "e2e", "n": n, "nb": nb, "dtype": dt}
    F = gj.batched.factor(A, dtype=dt)
    out["chunk"] = F.chunk
    out["factor_ms"] = wall_ms(lambda: gj.batched.factor(A, dtype=dt), reps)
    out["torch_inv_ms"] = wall_ms(lambda: torch.linalg.inv(A), reps)
    for k in (1, 16):
        B = torch.rand((nb, n, k), dtype=_DT[dt], device="cuda") - 0.5
        out[f"solve_k{k}_ms"] = wall_ms(lambda: F.solve(B), reps)
        out[f"solve_k{k}_sweeps_max"] = int(F.infos["steps"].max()) + 1
        out[f"solve_k{k}_converged"] = bool(F.infos["converged"].all())
        out[f"torch_solve_k{k}_ms"] = wall_ms(lambda: torch.linalg.solve(A, B), reps)
    # block_inverse alone on the packed panel of the whole stack
    m = max(n, 16)
    if nb * m * m * A.element_size() <= (1 << 30):
        Lt = torch.empty((m, nb * m), dtype=_DT[dt], device="cuda")
        norm = torch.empty(nb, dtype=torch.float64, device="cuda")
        exp = torch.empty(nb, dtype=torch.int32, device="cuda")
        ops.batch_pack(A.double(), Lt, norm, exp, m=m)
        bi = wall_ms(lambda: ops.block_inverse(Lt, nb * m, m, thresh=1e-15), reps)
        out["block_inverse_ms"] = bi
        out["outside"] = round(1.0 - bi / out["factor_ms"], 3)
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)


def kernels(n, nb, dt, reps):
    native = gj.load_native()
    d = ops.device_for(torch.empty(1, device="cuda"))
    m, es, k = max(n, 16), 8 if dt == "fp64" else 4, 16
    A = stack(n, nb, "fp64")
    Lt = torch.empty((m, nb * m), dtype=_DT[dt], device="cuda")
    inv_t = torch.rand((nb, m, m), dtype=_DT[dt], device="cuda")
    X = torch.empty((nb, n, n), dtype=_DT[dt], device="cuda")
    norm = torch.empty(nb, dtype=torch.float64, device="cuda")
    exp = torch.zeros(nb, dtype=torch.int32, device="cuda")
    valid = torch.ones(nb, dtype=torch.int32, device="cuda")
    V = torch.rand((nb, n, k), dtype=torch.float64, device="cuda")
    Y = torch.empty_like(V)
    torch.cuda.synchronize()
    runs = [("pack", (A, Lt, norm), nb * (n * n * 8 + m * m * es)),
            ("unpack", (inv_t, X, norm), nb * n * n * 2 * es),
            ("rhs", (X.normal_(), V, Y), nb * (n * n * es + 2 * n * k * 8))]
    for which, (a, b, c), nbytes in runs:
        us = d.time_batch_op(which, dt, a.data_ptr(), b.data_ptr(), c.data_ptr(), exp.data_ptr(), valid.data_ptr(), n, m,
                             nb, k, reps)
        cu = copy_us(nbytes, reps)
        print(json.dumps({"what": which, "n": n, "nb": nb, "dtype": dt, "kernel": native.last_batch_kernel(),
                          "us": round(us, 1), "GBps": round(nbytes / us / 1e3, 1), "copy_us": round(cu, 1),
                          "copy_GBps": round(nbytes / cu / 1e3, 1), "vs_copy": round(us / cu, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--dtypes", default="fp64,fp32")
    ap.add_argument("--only", choices=["e2e", "kernels"], default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_batched needs a GPU"
    warm = stack(32, 8, "fp64")
    gj.batched.factor(warm).solve(torch.rand((8, 32, 2), dtype=torch.float64, device="cuda"))
    torch.linalg.solve(warm, warm)
    for dt in a.dtypes.split(","):
        for n, nb in SHAPES:
            if a.only != "kernels":
                e2e(n, nb, dt, a.reps)
            if a.only != "e2e":
                kernels(n, nb, dt, a.kernel_reps)


if __name__ == "__main__":
    main()
