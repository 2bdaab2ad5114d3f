#!/usr/bin/env python3
"""What the error bounds of a refined solve cost on one GPU (profiles/error_bounds.md).

  kernel   Device::panel_abs_rhs and panel_abs_rhs_t alone (every column, column maxima on) next to
           their siblings panel_rhs / panel_rhs_t on the same P: device events over `--reps` launches
           after a warm-up launch; microseconds and achieved GB/s of P (the bytes of P over the time).
  solve    F = gj.factor(A) once per (n, dtype), then F.solve(B, trans=...) with and without
           bounds=True in turn, `--reps` times each after one warm-up of both: a host clock around a
           call that ends in a device synchronise; median, minimum and maximum in milliseconds.
           --no-bounds: only the solve without the option, so that the same script runs on the commit
           before this one (set PYTHONPATH to its tree) -- its repeats give the run-to-run spread the
           two commits are compared within.

n = 8192 and 32768 (--n to choose), fp64 and fp32, k = 1 / 16 / 64, plain and transposed.  One JSON
line per measurement."""
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

_DT = {"fp64": torch.float64, "fp32": torch.float32}
KS = (1, 16, 64)


def kernel(n, m, dt, k, reps):
    native = gj.load_native()
    dev = torch.device("cuda", 0)
    P = torch.rand((n, n), dtype=_DT[dt], device=dev) - 0.5
    V = torch.rand((n, k), dtype=torch.float64, device=dev) - 0.5
    Y = torch.zeros((n, k), dtype=torch.float64, device=dev)
    cm = torch.zeros(k, dtype=torch.float64, device=dev)
    d = ops.device_for(P)
    a = (dt, P.data_ptr(), n, n, m, 1, 0, V.data_ptr(), k, k, Y.data_ptr(), k)
    out = {"what": "kernel", "n": n, "m": m, "dtype": dt, "k": k, "reps": reps}
    gb = n * n * P.element_size() / 1e3  # bytes of P per microsecond -> GB/s
    for name, fn, probe, extra in (("panel_abs_rhs", d.time_panel_abs_rhs, native.last_abs_kernel, (cm.data_ptr(),)),
                                   ("panel_rhs", d.time_panel_rhs, native.last_rhs_kernel, (cm.data_ptr(),)),
                                   ("panel_abs_rhs_t", d.time_panel_abs_rhs_t, native.last_abs_kernel, ()),
                                   ("panel_rhs_t", d.time_panel_rhs_t, native.last_rhs_t_kernel, ())):
        us = fn(*a, *extra, reps)
        out[name] = {"us": round(us, 2), "P_GBps": round(gb / us, 1), "kernel": probe()}
    out["abs_over_plain"] = round(out["panel_abs_rhs"]["us"] / out["panel_rhs"]["us"], 3)
    out["abs_t_over_plain_t"] = round(out["panel_abs_rhs_t"]["us"] / out["panel_rhs_t"]["us"], 3)
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


def solve(n, m, dt, reps, with_bounds):
    from mpi_jordan_crazy_acceleration_amd.utils import generate_matrix
    dev = torch.device("cuda", 0)
    A64 = torch.from_numpy(generate_matrix(n, "randshift", 3)).to(dev, torch.float64)
    F = gj.factor(A64, block_size=m, dtype=dt)
    rng = np.random.default_rng(3)
    for k in KS:
        B = torch.from_numpy(rng.standard_normal((n, k))).to(dev)
        for trans in (False, True):
            # (k = 1, plain: without bounds the one-vector path, with bounds the block path as one column)
            Bk = B
            tr = {"trans": True} if trans else {}
            F.solve(Bk, **tr)  # warm-up: allocator, code objects
            out = {"what": "solve", "n": n, "m": m, "dtype": dt, "k": k, "trans": trans, "reps": reps}
            if with_bounds:
                F.solve(Bk, bounds=True, **tr)
            out["plain"] = _timed(F, Bk, reps, **tr)
            out["steps"] = max(i["steps"] for i in F.infos)
            out["converged"] = all(i["converged"] for i in F.infos)
            if with_bounds:
                out["bounds"] = _timed(F, Bk, reps, bounds=True, **tr)
                out["bounds_over_plain"] = round(out["bounds"]["median_ms"] / out["plain"]["median_ms"], 3)
                out["ferr_max"] = max(i["ferr"] for i in F.infos)
                out["berr_max"] = max(i["berr"] for i in F.infos)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "solve"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, nargs="*", default=[8192, 32768])
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--dtype", nargs="*", default=["fp64", "fp32"])
    ap.add_argument("--no-bounds", action="store_true")
    a = ap.parse_args()
    for n in a.n:
        for dt in a.dtype:
            if a.mode == "kernel":
                for k in KS:
                    print(json.dumps(kernel(n, a.m, dt, k, a.reps)), flush=True)
            else:
                solve(n, a.m, dt, a.reps, not a.no_bounds)
