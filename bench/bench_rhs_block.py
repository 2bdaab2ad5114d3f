#!/usr/bin/env python3
"""The block right-hand-side path on one GPU (profiles/rhs_block.md).

  kernel   Device::panel_rhs alone (Y = P V, column maxima on) against Device::gemm with N = k on
           the same operands, by device events over `--reps` launches after a warm-up launch:
           microseconds, achieved bytes/s of P, and the ratio.
  solve    gj.solve(A_cuda, B) end to end, the inversion timed apart from the right-hand sides.

One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mpi_jordan_crazy_acceleration_amd as gj  # noqa: E402
from mpi_jordan_crazy_acceleration_amd import ops  # noqa: E402

_DT = {"fp64": torch.float64, "fp32": torch.float32}


def kernel(n, m, dt, k, reps):
    dev = torch.device("cuda", 0)
    P = torch.rand((n, n), dtype=_DT[dt], device=dev) - 0.5
    V = torch.rand((n, k), dtype=torch.float64, device=dev) - 0.5
    Y = torch.zeros((n, k), dtype=torch.float64, device=dev)
    cm = torch.zeros(k, dtype=torch.float64, device=dev)
    d = ops.device_for(P)
    us = d.time_panel_rhs(dt, P.data_ptr(), n, n, m, 1, 0, V.data_ptr(), k, k, Y.data_ptr(), k, cm.data_ptr(), reps)
    name = gj.load_native().last_rhs_kernel()
    Vt, Ct = V.to(_DT[dt]), torch.zeros((n, k), dtype=_DT[dt], device=dev)
    torch.cuda.synchronize()
    us_g = d.time_gemm_store(dt, n, k, n, P.data_ptr(), n, Vt.data_ptr(), k, Ct.data_ptr(), k, reps)
    gname = gj.load_native().last_gemm_kernel()
    ref = P.double() @ V
    err = float((Y - ref).abs().max() / ref.abs().max())
    pbytes = n * n * P.element_size()
    return {"what": "kernel", "n": n, "m": m, "dtype": dt, "k": k, "reps": reps, "panel_rhs_us": round(us, 2),
            "panel_rhs_kernel": name, "P_TBps": round(pbytes / us / 1e6, 3), "gemm_us": round(us_g, 2),
            "gemm_kernel": gname, "gemm_P_TBps": round(pbytes / us_g / 1e6, 3), "gemm_over_rhs": round(us_g / us, 2),
            "rel_err": err}


def solve(n, m, dt, k, kind, seed):
    from mpi_jordan_crazy_acceleration_amd.utils import generate_matrix
    dev = torch.device("cuda", 0)
    A = torch.from_numpy(generate_matrix(n, kind, seed)).to(dev, torch.float64)
    B = torch.from_numpy(np.random.default_rng(seed).standard_normal((n, k))).to(dev)
    g = gj.GaussJordan(block_size=m, dtype=dt, residual="never")
    out = {"what": "solve", "n": n, "m": m, "dtype": dt, "k": k, "gen": kind}
    for rep in range(2):  # the first pass warms the allocator and the kernels up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g._inverse_resident(A)
        torch.cuda.synchronize()
        t_inv = time.perf_counter() - t0
        t0 = time.perf_counter()
        X, infos = g.solve_resident(A, B)
        torch.cuda.synchronize()
        t_all = time.perf_counter() - t0
    out.update(inverse_s=round(t_inv, 4), solve_resident_s=round(t_all, 4), rhs_s=round(t_all - t_inv, 4),
               converged=all(i["converged"] for i in infos), steps=[i["steps"] for i in infos],
               residual=float((A @ X - B).abs().max() / B.abs().max()))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "solve"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--dtype", default="fp32")
    a = ap.parse_args()
    if a.mode == "kernel":
        for n in (8192, 16384):
            for dt in ("fp64", "fp32"):
                for k in (1, 16, 64):
                    print(json.dumps(kernel(n, a.m, dt, k, a.reps)), flush=True)
    else:
        print(json.dumps(solve(a.n, a.m, a.dtype, a.k, "randshift", 3)), flush=True)
