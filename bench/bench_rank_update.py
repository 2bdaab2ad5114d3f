#!/usr/bin/env python3
"""The low-rank update of the resident inverse on one GPU (profiles/rank_update.md).

  kernel   Device::rank_update alone (X -= W Z^T and X += W Z^T in turn, W in local row order) by
           device events over `--reps` launches after two warm-up launches: microseconds, and the
           panel traffic it achieves (X read once and written once: 2 n^2 elements) in GB/s, set
           against the 6290 GB/s a float4 copy reaches on this GPU.
  e2e      F = gj.factor(A); then F.update(U, V) for k in {1, 16, 64} (host clock around a call that
           ends synchronised; the first call of a width warms up, the median of the next three is
           reported); then a fresh gj.factor(A + U V^T ...), which is all that could be done before
           this op existed.  One solve against the updated rows checks the result.

One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mpi_jordan_crazy_acceleration_amd as gj  # noqa: E402
from mpi_jordan_crazy_acceleration_amd import ops  # noqa: E402

_DT = {"fp64": torch.float64, "fp32": torch.float32}
COPY_GBPS = 6290.0


def kernel(n, m, dt, k, reps):
    native = gj.load_native()
    dev = torch.device("cuda", 0)
    X = torch.rand((n, n), dtype=_DT[dt], device=dev) - 0.5
    W = (torch.rand((n, k), dtype=torch.float64, device=dev) - 0.5) / k
    Z = torch.rand((n, k), dtype=torch.float64, device=dev) - 0.5
    ref = X[:256].double() - W[:256] @ Z.T
    d = ops.device_for(X)
    ops.rank_update(X, W, Z, n, m, sign=-1.0)
    err = float((X[:256].double() - ref).abs().max())
    ops.rank_update(X, W, Z, n, m, sign=1.0)
    us = d.time_rank_update(dt, X.data_ptr(), n, n, m, 1, 0, W.data_ptr(), k, Z.data_ptr(), k, k, reps)
    gbps = 2.0 * n * n * X.element_size() / us / 1e3
    return {"what": "kernel", "n": n, "m": m, "dtype": dt, "k": k, "reps": reps, "kernel": native.last_rank_update_kernel(),
            "us": round(us, 1), "panel_GBps": round(gbps, 1), "of_copy": round(gbps / COPY_GBPS, 3),
            "fp64_GFLOPs": round(2.0 * n * n * k / us / 1e3, 1), "abs_err": err}


def e2e(n, m, dt, ks):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    A = torch.rand((n, n), dtype=torch.float64, device=dev, generator=g) - 0.5
    A += float(n) ** 0.5 * torch.eye(n, dtype=torch.float64, device=dev)  # well conditioned at any n
    out = []

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    F, t_first = timed(lambda: gj.factor(A, block_size=m, dtype=dt))
    for k in ks:
        ts, info = [], None
        for rep in range(4):
            U = torch.randn((n, k), dtype=torch.float64, device=dev, generator=g) / float(n) ** 0.5
            V = torch.randn((n, k), dtype=torch.float64, device=dev, generator=g)
            info, t = timed(lambda: F.update(U, V))
            ts.append(t)
        med = sorted(ts[1:])[1]
        out.append({"what": "update", "n": n, "m": m, "dtype": dt, "k": k, "first_ms": round(1e3 * ts[0], 2),
                    "update_ms": round(1e3 * med, 2), "all_ms": [round(1e3 * t, 2) for t in ts],
                    "cond1": info["cond1"], "min_pivot": info["min_pivot"]})
    b = torch.randn((n, 4), dtype=torch.float64, device=dev, generator=g)
    x = F.solve(b)
    A2 = F._a64  # A plus every update, kept by the handle in fp64
    res = float((A2 @ x.double() - b).abs().max() / b.abs().max())
    conv = all(i["converged"] for i in F.infos)
    updates = F.updates
    A2 = A2.clone()
    del F
    ts = []
    for rep in range(2):
        G, t = timed(lambda: gj.factor(A2, block_size=m, dtype=dt))
        ts.append(t)
        del G
    refac = min(ts)
    for o in out:
        o["refactor_ms"] = round(1e3 * refac, 2)
        o["refactor_over_update"] = round(refac / (o["update_ms"] / 1e3), 1)
        print(json.dumps(o), flush=True)
    print(json.dumps({"what": "check", "n": n, "dtype": dt, "updates": updates, "solve_residual": res,
                      "converged": conv, "first_factor_ms": round(1e3 * t_first, 2),
                      "refactor_all_ms": [round(1e3 * t, 2) for t in ts]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "e2e"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, nargs="*", default=[8192, 32768])
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--k", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--dtype", nargs="*", default=["fp32", "fp64"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rank_update needs a GPU")
    for n in a.n:
        for dt in a.dtype:
            if a.mode == "kernel":
                for k in a.k:
                    print(json.dumps(kernel(n, a.m, dt, k, a.reps)), flush=True)
            else:
                e2e(n, a.m, dt, a.k)
