#!/usr/bin/env python3
"""Gradients from the resident inverse on one GPU (profiles/autograd.md).

  kernel   Device::grad_matrix alone by device events over `--reps` launches after a warm-up launch, for
           alpha only (k = 0), the product only (alpha = 0, k in --k) and both terms: microseconds, and the
           traffic it moves (G written once, 8 n^2 bytes; P read once where alpha != 0) in GB/s, set
           against a device-to-device copy that moves the same number of bytes (read + written), timed
           here by the same events.
  e2e      loss = 1/2 y^T inv(A) y + 1/2 log|det A| through one gj.autograd.factor: the forward alone and
           forward + backward (host clock around calls that end synchronised; a small problem warms every
           path up first, then the median of `--reps` runs), and the same loss through torch.linalg.solve
           and torch.linalg.slogdet on the same GPU in the engine's dtype.  The two gradients are compared.

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


def kernel(n, dt, k, alpha, reps, copies):
    native = gj.load_native()
    dev = torch.device("cuda", 0)
    P = torch.rand((n, n), dtype=_DT[dt], device=dev) - 0.5 if alpha != 0 else None
    G = torch.empty((n, n), dtype=torch.float64, device=dev)
    W = Z = None
    if k:
        W = (torch.rand((n, k), dtype=torch.float64, device=dev) - 0.5) / k
        Z = torch.rand((n, k), dtype=torch.float64, device=dev) - 0.5
    ops.grad_matrix(P, W, Z, G, n, alpha=alpha, sign=-1.0)
    ref = torch.zeros((256, n), dtype=torch.float64, device=dev)
    if alpha != 0:
        ref += alpha * P[:, :256].T.double()
    if k:
        ref -= W[:256] @ Z.T
    err = float((G[:256] - ref).abs().max())
    d = ops.device_for(G)
    us = d.time_grad_matrix(dt, P.data_ptr() if P is not None else 0, n, n, alpha, W.data_ptr() if k else 0, k,
                            Z.data_ptr() if k else 0, k, k, -1.0, False, G.data_ptr(), n, reps)
    nbytes = 8 * n * n + (P.element_size() * n * n if P is not None else 0)
    if nbytes not in copies:
        del P, ref
        copies[nbytes] = copy_us(nbytes, reps)
    cus = copies[nbytes]
    return {"what": "kernel", "n": n, "dtype": dt if alpha != 0 else "-", "k": k, "alpha": alpha, "reps": reps,
            "kernel": native.last_grad_matrix_kernel(), "us": round(us, 1), "GBps": round(nbytes / us / 1e3, 1),
            "copy_us": round(cus, 1), "copy_GBps": round(nbytes / cus / 1e3, 1), "of_copy": round(cus / us, 3),
            "fp64_GFLOPs": round(2.0 * n * n * k / us / 1e3, 1), "abs_err": err}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def _ours(A, y, m, dt):
    A = A.detach().requires_grad_()

    def fwd():
        F = gj.autograd.factor(A, block_size=m, dtype=dt)
        return 0.5 * (y @ F.solve(y)) + 0.5 * F.slogdet()[1]

    loss, tf = _timed(fwd)
    _, tb = _timed(loss.backward)
    return float(loss.detach()), A.grad, tf, tb


def _torch(A, y, dt):
    A = A.detach().to(_DT[dt]).requires_grad_()
    yy = y.to(_DT[dt])

    def fwd():
        return 0.5 * (yy @ torch.linalg.solve(A, yy)) + 0.5 * torch.linalg.slogdet(A)[1]

    loss, tf = _timed(fwd)
    _, tb = _timed(loss.backward)
    return float(loss.detach()), A.grad, tf, tb


def _problem(n):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    A = torch.rand((n, n), dtype=torch.float64, device=dev, generator=g) - 0.5
    A += float(n) ** 0.5 * torch.eye(n, dtype=torch.float64, device=dev)  # well conditioned at any n
    y = torch.rand((n,), dtype=torch.float64, device=dev, generator=g) - 0.5
    return A, y


def e2e(n, m, dt, reps):
    A, y = _problem(1024)  # every path once, small
    _ours(A, y, m, dt)
    _torch(A, y, dt)
    A, y = _problem(n)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    ours = [_ours(A, y, m, dt) for _ in range(reps)]
    g_ours = ours[-1][1].double()
    ours = [(o[0], None, o[2], o[3]) for o in ours]
    ref = [_torch(A, y, dt) for _ in range(reps)]
    g_ref = ref[-1][1].double()
    rel = float((g_ours - g_ref).abs().max() / g_ref.abs().max())
    print(json.dumps({"what": "e2e", "n": n, "m": m, "dtype": dt, "reps": reps,
                      "fwd_ms": round(1e3 * med([o[2] for o in ours]), 2),
                      "bwd_ms": round(1e3 * med([o[3] for o in ours]), 2),
                      "fwd_bwd_ms": round(1e3 * med([o[2] + o[3] for o in ours]), 2),
                      "torch_fwd_ms": round(1e3 * med([o[2] for o in ref]), 2),
                      "torch_bwd_ms": round(1e3 * med([o[3] for o in ref]), 2),
                      "torch_fwd_bwd_ms": round(1e3 * med([o[2] + o[3] for o in ref]), 2),
                      "loss": ours[-1][0], "torch_loss": ref[-1][0], "grad_rel_diff": rel}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "e2e"])
    ap.add_argument("--reps", type=int, default=0, help="0: 20 launches (kernel), 3 runs (e2e)")
    ap.add_argument("--n", type=int, nargs="*", default=[8192, 32768])
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--k", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--dtype", nargs="*", default=["fp32", "fp64"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_autograd needs a GPU")
    for n in a.n:
        if a.mode == "kernel":
            reps, copies = a.reps or 20, {}
            for k in a.k:  # the product alone: P is not read, no dtype
                print(json.dumps(kernel(n, "fp64", k, 0.0, reps, copies)), flush=True)
            for dt in a.dtype:
                print(json.dumps(kernel(n, dt, 0, 1.0, reps, copies)), flush=True)  # alpha only
                for k in a.k:
                    print(json.dumps(kernel(n, dt, k, -0.375, reps, copies)), flush=True)  # both terms
        else:
            for dt in a.dtype:
                e2e(n, a.m, dt, a.reps or 3)
