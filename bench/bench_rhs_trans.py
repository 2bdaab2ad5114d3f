#!/usr/bin/env python3
"""The transposed right-hand-side path on one GPU (profiles/rhs_trans.md).

  kernel   Device::panel_rhs_t alone (S = P^T V, every column active) against Device::panel_rhs on
           the same P (Y = P V: the same bytes streamed, the rate a kernel of this family reaches)
           and against Device::gemm (Store, K-major A = P, N = k, V already converted to P's type),
           by device events over `--reps` launches after a warm-up launch: microseconds, achieved
           bytes/s of P, and the ratios.
  e2e      a forward solve of B plus a transposed solve of C, n x k each:
             --route factor      F = gj.factor(A); F.solve(B); F.solve(C, trans=True)   (one inversion)
             --route two-solves  gj.solve(A, B); gj.solve(A.T.contiguous(), C)           (two; runs on
                                 the commit before this one as well)

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
    native = gj.load_native()
    dev = torch.device("cuda", 0)
    P = torch.rand((n, n), dtype=_DT[dt], device=dev) - 0.5
    V = torch.rand((n, k), dtype=torch.float64, device=dev) - 0.5
    S = torch.zeros((n, k), dtype=torch.float64, device=dev)
    Y = torch.zeros((n, k), dtype=torch.float64, device=dev)
    cm = torch.zeros(k, dtype=torch.float64, device=dev)
    d = ops.device_for(P)
    us_t = d.time_panel_rhs_t(dt, P.data_ptr(), n, n, m, 1, 0, V.data_ptr(), k, k, S.data_ptr(), k, reps)
    name_t = native.last_rhs_t_kernel()
    us_f = d.time_panel_rhs(dt, P.data_ptr(), n, n, m, 1, 0, V.data_ptr(), k, k, Y.data_ptr(), k, cm.data_ptr(), reps)
    name_f = native.last_rhs_kernel()
    Vt, Ct = V.to(_DT[dt]), torch.zeros((n, k), dtype=_DT[dt], device=dev)
    torch.cuda.synchronize()
    us_g = d.time_gemm_store_kmajor(dt, n, k, n, P.data_ptr(), n, Vt.data_ptr(), k, Ct.data_ptr(), k, reps)
    gname = native.last_gemm_kernel()
    ref = P.double().T @ V
    err = float((S - ref).abs().max() / ref.abs().max())
    gerr = float((Ct.double() - ref).abs().max() / ref.abs().max())
    pbytes = n * n * P.element_size()
    return {"what": "kernel", "n": n, "m": m, "dtype": dt, "k": k, "reps": reps,
            "panel_rhs_t_us": round(us_t, 2), "panel_rhs_t_kernel": name_t, "P_TBps": round(pbytes / us_t / 1e6, 3),
            "panel_rhs_us": round(us_f, 2), "panel_rhs_kernel": name_f,
            "panel_rhs_P_TBps": round(pbytes / us_f / 1e6, 3),
            "t_over_plain": round(us_t / us_f, 2),
            "gemm_us": round(us_g, 2), "gemm_kernel": gname, "gemm_P_TBps": round(pbytes / us_g / 1e6, 3),
            "gemm_over_t": round(us_g / us_t, 2), "rel_err": err, "gemm_rel_err": gerr}


def e2e(n, m, dt, k, kind, seed, route):
    from mpi_jordan_crazy_acceleration_amd.utils import generate_matrix
    dev = torch.device("cuda", 0)
    # A is an fp64 tensor on both routes (the engine converts it to its own dtype), so X comes back in fp64
    A64 = torch.from_numpy(generate_matrix(n, kind, seed)).to(dev, torch.float64)
    rng = np.random.default_rng(seed)
    B = torch.from_numpy(rng.standard_normal((n, k))).to(dev)
    C = torch.from_numpy(rng.standard_normal((n, k))).to(dev)
    out = {"what": "e2e", "route": route, "n": n, "m": m, "dtype": dt, "k": k, "gen": kind}
    for rep in range(2):  # the first pass warms the allocator and the kernels up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if route == "factor":
            F = gj.factor(A64, block_size=m, dtype=dt)
            X = F.solve(B)
            Xt = F.solve(C, trans=True)
        else:
            X = gj.solve(A64, B, block_size=m, dtype=dt)
            Xt = gj.solve(A64.T.contiguous(), C, block_size=m, dtype=dt)
        torch.cuda.synchronize()
        t_all = time.perf_counter() - t0
    out.update(seconds=round(t_all, 4), x_dtype=str(X.dtype),
               residual=float((A64 @ X.double() - B).abs().max() / B.abs().max()),
               residual_t=float((A64.T @ Xt.double() - C).abs().max() / C.abs().max()))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "e2e"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--route", choices=["factor", "two-solves"], default="factor")
    a = ap.parse_args()
    if a.mode == "kernel":
        for n in (8192, 16384):
            for dt in ("fp64", "fp32"):
                for k in (1, 16, 64):
                    print(json.dumps(kernel(n, a.m, dt, k, a.reps)), flush=True)
    else:
        print(json.dumps(e2e(a.n, a.m, a.dtype, a.k, "randshift", 3, a.route)), flush=True)
