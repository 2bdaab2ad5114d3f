#!/usr/bin/env python3
"""What the determinant costs on one GPU (profiles/slogdet.md).

  overhead  one inversion (generate + solve, bench.py's step) with SolveOptions::track_det off, on and
            off again, `--warmup` untimed and `--steps` timed steps each (bench.py's defaults): the
            mean, the median and the fastest step.  The second "off" run shows the run-to-run spread
            the on - off difference has to be read against.  `--off-only` skips the tracked run and
            never names the option, so the same file measures a checkout that does not have it.
  call      Engine::slogdet alone after a tracked inversion (its own `seconds`, a fresh inversion
            before every call: the value is cached), and Device::slogdet_batch alone on Nr random
            blocks (host clock around a call that ends synchronised, the fastest of `--reps`).
  host      numpy.linalg.slogdet of the same matrix on the host, for scale, and the engine's value
            against it.

One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mpi_jordan_crazy_acceleration_amd as gj  # noqa: E402

SEED = 2024  # bench.py's


def _engine(n, m, dt, track):
    C = gj.load_native()
    kw = {} if track is None else {"track_det": bool(track)}
    return C.Engine(C.hip_device(0), C.self_comm(), n, m, dt, **kw)


def _steps(eng, count):
    ms = []
    for _ in range(count):
        t0 = time.perf_counter()
        eng.generate("random", SEED)
        st = eng.solve()  # returns after the device has finished
        ms.append((time.perf_counter() - t0) * 1e3)
        if st["status"] != 0:
            sys.exit(f"solve failed with status {st['status']}")
    return ms


def overhead(n, m, dt, warmup, steps, off_only):
    runs = [("off", None)] if off_only else [("off", False), ("on", True), ("off again", False)]
    for name, track in runs:
        eng = _engine(n, m, dt, track)
        _steps(eng, warmup)
        ms = _steps(eng, steps)
        del eng
        print(json.dumps({"what": "overhead", "n": n, "m": m, "dtype": dt, "track_det": name, "warmup": warmup,
                          "steps": steps, "mean_ms": round(statistics.fmean(ms), 2),
                          "median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2),
                          "max_ms": round(max(ms), 2)}), flush=True)


def call(n, m, dt, reps):
    from mpi_jordan_crazy_acceleration_amd import ops

    native = gj.load_native()
    eng = _engine(n, m, dt, True)
    secs, solve_ms = [], []
    for _ in range(reps):
        solve_ms += _steps(eng, 1)
        d = eng.slogdet()
        if d["status"] != 0:
            sys.exit(f"slogdet failed with status {d['status']}")
        secs.append(d["seconds"])
    name = native.last_slogdet_kernel()
    nr = -(-n // m)
    print(json.dumps({"what": "Engine.slogdet", "n": n, "m": m, "dtype": dt, "blocks": nr, "kernel": name,
                      "call_ms": [round(1e3 * s, 3) for s in secs], "solve_ms": [round(t, 1) for t in solve_ms],
                      "sign": d["sign"], "logabsdet": d["logabsdet"]}), flush=True)
    del eng
    tdt = torch.float64 if dt == "fp64" else torch.float32
    B = torch.randn((nr, m, m), dtype=tdt, device="cuda")
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.slogdet_batch(B)
        ts.append(time.perf_counter() - t0)
    print(json.dumps({"what": "slogdet_batch", "m": m, "dtype": dt, "blocks": nr, "kernel": native.last_slogdet_kernel(),
                      "first_ms": round(1e3 * ts[0], 3), "min_ms": round(1e3 * min(ts[1:]), 3)}), flush=True)


def host(n, m, dt):
    g = torch.Generator(device="cuda").manual_seed(3)
    A = torch.rand((n, n), dtype=torch.float64, device="cuda", generator=g) - 0.5
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    F = gj.factor(A, block_size=m, dtype=dt)
    sign, logabs = F.slogdet()
    t_gj = time.perf_counter() - t0
    del F
    a = A.cpu().numpy()
    del A
    t0 = time.perf_counter()
    rs, rl = np.linalg.slogdet(a)
    t_np = time.perf_counter() - t0
    print(json.dumps({"what": "host", "n": n, "m": m, "dtype": dt, "numpy_slogdet_s": round(t_np, 2),
                      "factor_plus_slogdet_s": round(t_gj, 2), "sign": sign, "numpy_sign": float(rs),
                      "logabsdet": logabs, "abs_dlog": abs(logabs - float(rl)),
                      "threads": os.environ.get("OMP_NUM_THREADS", "")}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["overhead", "call", "host"])
    ap.add_argument("--n", type=int, nargs="*", default=[8192, 32768])
    ap.add_argument("--m", type=int, nargs="*", default=[128])
    ap.add_argument("--dtype", default="fp64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--off-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_slogdet needs a GPU")
    for n in a.n:
        for m in a.m:
            if a.mode == "overhead":
                overhead(n, m, a.dtype, a.warmup, a.steps, a.off_only)
            elif a.mode == "call":
                call(n, m, a.dtype, a.reps)
            else:
                host(n, m, a.dtype)
