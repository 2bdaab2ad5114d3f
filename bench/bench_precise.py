#!/usr/bin/env python3
"""What extra-precise refinement costs on one GPU (profiles/precise_refine.md).

  kernel   Device::panel_rhs_dd (the double-double residual, every column, column maxima on) next to
           panel_rhs (fp64) on the same P: device events over `--reps` launches after a warm-up launch;
           microseconds and achieved GB/s of P (the bytes of P over the time).
  solve    F = gj.factor(A) once per n (fp64 engine), then F.solve(B) with and without precise=True in
           turn, `--reps` times each after one warm-up of both: a host clock around a call that ends in
           a device synchronise; median, minimum and maximum in milliseconds.
           --no-precise: only the solve without the option, so that the same script runs on the commit
           before this one (set PYTHONPATH to its tree) -- its repeats give the run-to-run spread the
           two commits are compared within.

n = 8192 and 32768 (--n to choose), k = 1 / 16 / 64.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

if "PYTHONPATH" not in os.environ:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mpi_jordan_crazy_acceleration_amd as gj  # noqa: E402
from mpi_jordan_crazy_acceleration_amd import ops  # noqa: E402

KS = (1, 16, 64)


def kernel(n, m, k, reps):
    native = gj.load_native()
    dev = torch.device("cuda", 0)
    P = torch.rand((n, n), dtype=torch.float64, device=dev) - 0.5
    V = torch.rand((n, k), dtype=torch.float64, device=dev) - 0.5
    Y = torch.zeros((n, k), dtype=torch.float64, device=dev)
    cm = torch.zeros(k, dtype=torch.float64, device=dev)
    d = ops.device_for(P)
    a = (P.data_ptr(), n, n, m, 1, 0, V.data_ptr(), k, k, Y.data_ptr(), k, cm.data_ptr(), reps)
    out = {"what": "kernel", "n": n, "m": m, "k": k, "reps": reps}
    gb = n * n * 8 / 1e3  # bytes of P per microsecond -> GB/s
    us = d.time_panel_rhs_dd(*a)
    out["panel_rhs_dd"] = {"us": round(us, 2), "P_GBps": round(gb / us, 1), "kernel": native.last_rhs_dd_kernel()}
    us = d.time_panel_rhs("fp64", *a)
    out["panel_rhs"] = {"us": round(us, 2), "P_GBps": round(gb / us, 1), "kernel": native.last_rhs_kernel()}
    out["dd_over_plain"] = round(out["panel_rhs_dd"]["us"] / out["panel_rhs"]["us"], 2)
    # Dot2 is 10 fp64 vector operations per multiply-add
    out["dd_vector_Tops"] = round(10.0 * n * n * max(k, 16 if k <= 16 else 32 if k <= 32 else 64) /
                                  out["panel_rhs_dd"]["us"] / 1e6, 2)
    return out


def _timed(F, B, reps, **kw):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        F.solve(B, **kw)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def solve(n, m, reps, with_precise):
    from mpi_jordan_crazy_acceleration_amd.utils import generate_matrix
    dev = torch.device("cuda", 0)
    A64 = torch.from_numpy(generate_matrix(n, "randshift", 3)).to(dev, torch.float64)
    F = gj.factor(A64, block_size=m, dtype="fp64")
    rng = np.random.default_rng(3)
    for k in KS:
        # (k = 1: without the option the one-vector path, with it the block path as one column)
        B = torch.from_numpy(rng.standard_normal((n, k))).to(dev)
        F.solve(B)  # warm-up: allocator, code objects
        out = {"what": "solve", "n": n, "m": m, "k": k, "reps": reps}
        if with_precise:
            F.solve(B, precise=True)
        out["plain"] = _timed(F, B, reps)
        out["steps"] = max(i["steps"] for i in F.infos)
        if with_precise:
            out["precise"] = _timed(F, B, reps, precise=True)
            out["precise_over_plain"] = round(out["precise"]["median_ms"] / out["plain"]["median_ms"], 3)
            out["precise_steps"] = max(i["steps"] for i in F.infos)
            out["converged"] = all(i["converged"] for i in F.infos)
            out["err_est_max"] = max(i["err_est"] for i in F.infos)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "solve"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, nargs="*", default=[8192, 32768])
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--no-precise", action="store_true")
    a = ap.parse_args()
    for n in a.n:
        if a.mode == "kernel":
            for k in KS:
                print(json.dumps(kernel(n, a.m, k, a.reps)), flush=True)
        else:
            solve(n, a.m, a.reps, not a.no_precise)
