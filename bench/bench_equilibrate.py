#!/usr/bin/env python3
"""The power-of-two equilibration on one GPU (profiles/equilibrate.md).

  kernel   Device::abs_max_rows, abs_max_cols and scale_pow2 alone, by device events over `--reps`
           launches after two warm-up launches: microseconds, and the panel traffic each achieves (the
           maxima read X once, n^2 elements; the scaling reads and writes it, 2 n^2) in GB/s, set
           against the 6290 GB/s a float4 copy reaches on this GPU.  scale_pow2 runs with the
           non-temporal policy (the default) and with plain accesses; its exponents alternate in sign
           from launch to launch, so that X stays bounded.
  whole    bench.py's step (fill the input panel, then Engine::solve; host clock around a step that ends
           synchronised) with the option off and on, alternating, `--steps` of each after `--warmup`:
             random   the benchmark's generator: the exponents are uniform and non-zero, all four
                      passes run
             scaled   ldexp(B, er[i] + ec[j]), B well conditioned, er, ec in -40 .. 40, uploaded from a
                      device tensor; the plain sweep calls it singular, so "off" inverts the same
                      matrix equilibrated by hand (what a user had to do without the option)

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
COPY_GBPS = 6290.0


def kernel(n, m, dt, reps):
    native = gj.load_native()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    X = torch.rand((n, n), dtype=_DT[dt], device=dev, generator=g) - 0.5
    e = lambda: torch.randint(-8, 9, (n,), dtype=torch.int32, device=dev, generator=g)
    rexp, cexp = e(), e()
    nr, nc = (-rexp).contiguous(), (-cexp).contiguous()
    out = torch.zeros(n, dtype=torch.float64, device=dev)
    d = ops.device_for(X)
    # the result first: the maxima against torch, the scaling there and back bit for bit
    ops.abs_max_rows(X, out, n, m)
    ok = bool(torch.equal(out, X.abs().max(dim=1).values.double()))
    ops.abs_max_cols(X, out, n, m, rexp_nat=rexp)
    ok = ok and bool(torch.equal(out, torch.ldexp(X.abs().double(), rexp[:, None]).max(dim=0).values))
    X0 = X.clone()
    ops.scale_pow2(X, n, m, rexp_nat=rexp, cexp=cexp)
    ops.scale_pow2(X, n, m, rexp_nat=nr, cexp=nc)
    ok = ok and bool(torch.equal(X, X0))
    del X0
    es = X.element_size()
    for which, passes, nt in (("rmax", 1, None), ("cmax", 1, None), ("scale", 2, True), ("scale", 2, False)):
        if nt is not None:
            native.set_equil_nt(nt)
        us = d.time_equil(which, dt, X.data_ptr(), n, n, m, rexp.data_ptr(), cexp.data_ptr(), nr.data_ptr(),
                          nc.data_ptr(), out.data_ptr(), reps)
        native.set_equil_nt(True)
        gbps = passes * n * n * es / us / 1e3
        rec = {"what": "kernel", "op": which, "n": n, "m": m, "dtype": dt, "reps": reps,
               "kernel": native.last_equil_kernel(), "us": round(us, 1), "panel_GBps": round(gbps, 1),
               "of_copy": round(gbps / COPY_GBPS, 3), "results_ok": ok}
        if nt is not None:
            rec["non_temporal"] = nt
        print(json.dumps(rec), flush=True)


def whole(n, m, dt, steps, warmup, inputs):
    C = gj.load_native()
    dev = torch.device("cuda", 0)
    hip = C.hip_device(0)
    eng = {on: C.Engine(hip, C.self_comm(), n, m, dt, equilibrate=on) for on in (False, True)}

    def run(fill):
        ts = {False: [], True: []}
        st = {}
        for i in range(warmup + steps):
            for on in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fill(eng[on], on)
                st[on] = eng[on].solve()
                t = time.perf_counter() - t0
                if st[on]["status"] != 0:
                    sys.exit(f"solve failed: status {st[on]['status']} (equilibrate={on})")
                if i >= warmup:
                    ts[on].append(1e3 * t)
        return ts, st

    def report(name, ts, st, extra=None):
        rec = {"what": "whole", "input": name, "n": n, "m": m, "dtype": dt, "steps": steps, "warmup": warmup}
        for on, key in ((False, "off"), (True, "on")):
            rec[key + "_ms_median"] = round(statistics.median(ts[on]), 2)
            rec[key + "_ms_min"] = round(min(ts[on]), 2)
            rec[key + "_ms_max"] = round(max(ts[on]), 2)
        rec["on_minus_off_ms"] = round(rec["on_ms_median"] - rec["off_ms_median"], 2)
        rec["equilibrate"] = {k: (list(v) if isinstance(v, tuple) else v) for k, v in st[True]["equilibrate"].items()}
        rec.update(extra or {})
        print(json.dumps(rec), flush=True)

    if "random" in inputs:
        ts, st = run(lambda e, on: e.generate("random", 0))
        norm_a, norm_inv = eng[True].input_norm_inf(), eng[True].result_norm_inf()
        res = eng[True].residual_generated("random", 0)
        report("random", ts, st, {"on_residual": res, "on_rho_over_n": res / (norm_a * norm_inv * (
            2.0 ** -52 if dt == "fp64" else 2.0 ** -23)) / n})
    if "scaled" in inputs:
        g = torch.Generator(device=dev).manual_seed(3)
        A = torch.rand((n, n), dtype=torch.float64, device=dev, generator=g) - 0.5
        A += float(n) ** 0.5 * torch.eye(n, dtype=torch.float64, device=dev)
        A = A.to(_DT[dt])
        er = torch.randint(-40, 41, (n,), dtype=torch.int32, device=dev, generator=g)
        ec = torch.randint(-40, 41, (n,), dtype=torch.int32, device=dev, generator=g)
        ops.scale_pow2(A, n, m, rexp_nat=er, cexp=ec)
        # by hand: the rule with torch, the matrix "off" gets
        r = 1 - torch.frexp(A.abs().max(dim=1).values.double())[1]
        As = torch.ldexp(A, r[:, None])
        c = 1 - torch.frexp(As.abs().max(dim=0).values.double())[1]
        As = torch.ldexp(As, c[None, :]).to(_DT[dt])
        torch.cuda.synchronize()
        mats = {False: As, True: A}
        ts, st = run(lambda e, on: e.upload_rows_device(mats[on].data_ptr(), n))
        q = eng[True].equil_exponents()
        same = bool((torch.from_numpy(q["row_exp"]).to(dev) == r).all() and (torch.from_numpy(q["col_exp"]).to(dev) == c).all())
        report("scaled", ts, st, {"exponents_match_torch": same})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "whole"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--dtype", nargs="*", default=["fp64", "fp32"])
    ap.add_argument("--input", nargs="*", default=["random", "scaled"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_equilibrate needs a GPU")
    for dt in a.dtype:
        if a.mode == "kernel":
            kernel(a.n, a.m, dt, a.reps)
        else:
            whole(a.n, a.m, dt, a.steps, a.warmup, a.input)
