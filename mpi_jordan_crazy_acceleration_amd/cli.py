"""Reference-compatible front end for the one-process-per-GPU deployment.

    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m mpi_jordan_crazy_acceleration_amd.cli \\
        [options] n m [file]

The ``mpirun -np p ./a.out n m [file]`` contract of the reference (main.cpp:65-93, solve()
:343-519) over ``torch.distributed``: one rank per process (RCCL on GPUs, gloo + the native host
executor with ``--device cpu``), every rank parsing only its own block rows of ``file``
(``DistributedGaussJordan.load_file``).  Rank 0 prints exactly what the reference prints: ``A`` and
its corner, ``glob_time: %.2f`` (max over ranks), ``inverse matrix:`` + blank line, the inverse's
corner, ``residual: %e`` (or ``p == 1!`` with ``--residual compat`` on one rank).  Exit codes:
0 ok, 1 usage, 2 any failure (cannot open / cannot read / singular matrix / not enough memory).
The in-process ``build/gj`` binary is the same contract with threads instead of processes.
``--det``: one more line after the residual line, ``slogdet: <sign> <logabsdet>`` (the determinant
from the pivot blocks, ``DistributedGaussJordan.slogdet``), and ``"slogdet"`` in ``--json``.
``--equilibrate``: power-of-two row and column scaling ahead of the sweep, undone on the inverse
(``DistributedGaussJordan(equilibrate=True)``); stdout keeps its form (the A corner is the matrix as
given, the residual is against it) and ``--json`` gains ``"equilibrate"``.
``--rhs ones|random`` with ``--nrhs K``, ``--trans``, ``--bounds``: the right-hand sides of ``build/gj``
(column j is (j+1) * ones, or seeded by seed + j), solved as a block by
``DistributedGaussJordan.solve_rhs`` -- ``solution x:``, the head of column 0 and ``Ax-b residual: %e``
(``ATx-b`` with ``--trans``; the maximum over the columns) as there; ``--bounds`` leaves stdout alone and
adds ``"axb_ferr_cols"`` / ``"axb_berr_cols"`` to ``--json``.  (One right-hand side without ``--trans``
or ``--bounds`` runs the one-vector path in ``build/gj`` and the block path here.)  With a file the
fp64 residual re-reads the rank's rows from it.
``--precise`` with ``--rhs``: extra-precise refinement, the residual accumulated in twice the working
precision (``solve_rhs(precise=True)``); stdout keeps its form and ``--json`` gains ``"precise": true``,
``"axb_dx_rel_cols"`` and ``"axb_err_est_cols"``.  Not with ``--trans`` (usage, exit 1).
``--cond``: one more line ``cond: %e %e`` (kappa_1 and kappa_inf, ``DistributedGaussJordan.cond``) after
the residual line, and after the slogdet line when both are given; ``"cond": {"one", "inf"}`` in
``--json``.
``--comm-timeout S``: a rank waiting longer than S seconds on a peer fails (every rank, naming the
step, phase and collective).  ``--same-gpu``: rehearse the p-rank RCCL path with every rank on
GPU 0 (each rank its own RCCL host over loopback sockets; functional check, not a timing).
"""
from __future__ import annotations

import json
import os
import sys


def _usage(prog: str) -> int:
    print(f"usage:{prog} n m [<file>]", flush=True)
    return 1


def _atoi(s: str) -> int:
    # C atoi: optional sign + leading digits, 0 when there are none
    s = s.strip()
    i, sign = 0, 1
    if i < len(s) and s[i] in "+-":
        sign = -1 if s[i] == "-" else 1
        i += 1
    j = i
    while j < len(s) and s[j].isdigit():
        j += 1
    return sign * int(s[i:j]) if j > i else 0


def _corner(c) -> str:
    return "".join("".join(f"{v:.2f}\t" for v in row) + "\n" for row in c)


def _rhs_block(kind: str, n: int, nrhs: int, seed: int):
    """The right-hand sides of build/gj --rhs ones|random --nrhs K (csrc/solver/runner.cpp): column j is
    (j + 1) * ones, or column 0 of the "random" generator seeded by (seed + j) ^ 0x9E3779B97F4A7C15."""
    import numpy as np

    from .utils.reference import _MASK, _splitmix64

    if kind == "ones":
        return np.tile(np.arange(1, nrhs + 1, dtype=np.float64), (n, 1))
    B = np.empty((n, nrhs))
    i = np.arange(n, dtype=np.uint64)
    for j in range(nrhs):
        sj = ((seed + j) & _MASK) ^ 0x9E3779B97F4A7C15
        with np.errstate(over="ignore"):
            s = (np.uint64(sj) * np.uint64(0x2545F4914F6CDD1D)) & np.uint64(_MASK)
            h = _splitmix64(s ^ (i << np.uint64(32)))
        B[:, j] = (h >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0
    return B


def main(argv=None) -> int:
    import argparse

    argv = sys.argv[1:] if argv is None else argv
    prog = "gj"
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    ap.add_argument("pos", nargs="*")
    ap.add_argument("--device", choices=["auto", "gpu", "cpu"], default="auto")
    ap.add_argument("--dtype", choices=["fp64", "fp32"], default="fp64")
    ap.add_argument("--gen", choices=["absdiff", "hilbert", "random", "randshift", "identity"], default="absdiff")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--residual", choices=["always", "compat", "never"], default="always")
    ap.add_argument("--print-max", type=int, default=10)
    ap.add_argument("--eps", type=float, default=1e-15)
    ap.add_argument("--depth", type=int, default=0)
    ap.add_argument("--pivot", choices=["block-min-inv-norm", "partial"], default="block-min-inv-norm")
    ap.add_argument("--chunk-cols", type=int, default=0)
    ap.add_argument("--host-threads", type=int, default=0)
    ap.add_argument("--comm-timeout", type=float, default=600.0)
    ap.add_argument("--bcast", choices=["auto", "ring", "direct"], default=None)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--det", action="store_true")
    ap.add_argument("--equilibrate", action="store_true")
    ap.add_argument("--same-gpu", action="store_true")
    ap.add_argument("--rhs", choices=["ones", "random"], default=None)
    ap.add_argument("--nrhs", type=int, default=1)
    ap.add_argument("--trans", action="store_true")
    ap.add_argument("--bounds", action="store_true")
    ap.add_argument("--precise", action="store_true")
    ap.add_argument("--cond", action="store_true")
    try:
        args, unknown = ap.parse_known_args(argv)
    except SystemExit:
        return _usage(prog)
    if unknown or not (2 <= len(args.pos) <= 3):
        return _usage(prog)
    n, m = _atoi(args.pos[0]), _atoi(args.pos[1])
    if n <= 0 or m <= 0 or args.print_max < 0 or args.nrhs < 1 or (args.trans and args.precise):
        return _usage(prog)
    path = args.pos[2] if len(args.pos) == 3 else None
    if args.bcast:
        os.environ["GJ_BCAST"] = args.bcast

    from .runtime_env import configure_runtime_env

    configure_runtime_env()
    import torch
    import torch.distributed as dist

    from ._native import load_native
    from .parallel.dist import DistributedGaussJordan

    C = load_native()
    gpu = args.device == "gpu" or (args.device == "auto" and C.device_count() > 0)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.same_gpu:
        # rehearsal of the p-rank RCCL path on ONE GPU (as bench.py --same-gpu): every rank is its
        # own RCCL "host", so RCCL accepts the shared device and connects the ranks by sockets
        local = 0
        os.environ["NCCL_HOSTID"] = f"gj-cli-rank{rank}"
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
        os.environ.setdefault("NCCL_IB_DISABLE", "1")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    from datetime import timedelta

    pg_timeout = timedelta(seconds=max(60.0, args.comm_timeout))
    if gpu:
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local), rank=rank, world_size=world,
                                timeout=pg_timeout)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=pg_timeout)
    out = (lambda s: print(s, end="", flush=True)) if rank == 0 else (lambda s: None)
    nm = min(n, args.print_max)
    try:
        try:
            solver = DistributedGaussJordan(n, m, dtype=args.dtype, chunk_cols=args.chunk_cols, eps=args.eps,
                                            host_threads=args.host_threads, depth=args.depth, pivot=args.pivot,
                                            local_rank=local if gpu else None, comm_timeout=args.comm_timeout,
                                            det=args.det, equilibrate=args.equilibrate)
        except C.GJError as e:  # agreed on every rank inside the constructor
            out("Not enough memory!\n" if e.status == 2 else f"error: {e}\n")
            return 2
        if path is not None:
            try:
                solver.load_file(path, args.host_threads)
            except FileNotFoundError:
                out(f"cannot open {path}\n")
                return 2
            except ValueError:
                out(f"cannot read {path}\n")
                return 2
        else:
            solver.generate(args.gen, args.seed)
        out("A\n" + _corner(solver.corner(nm, "input")))
        try:
            st = solver.solve()
        except C.GJError as e:
            if e.status != 6:  # not a communication failure
                raise
            # a peer died or hung: every rank names its step, phase and collective (Engine::solve)
            # and leaves at once -- tearing the process group down could block on the dead peer
            print(f"gj: rank {rank}: {e}", file=sys.stderr, flush=True)
            os._exit(2)
        if st["status"] != 0:
            out("singular matrix\n" if st["status"] == 1 else
                "not enough memory for block\n" if st["status"] == 7 else f"unknown error: {st['status']}\n")
            return 2
        t = torch.tensor([st["seconds"]], dtype=torch.float64, device="cuda" if gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        glob = float(t.item())
        out(f"glob_time: {glob:.2f}\ninverse matrix:\n\n" + _corner(solver.corner(nm, "result")))
        want_res = args.residual == "always" or (args.residual == "compat" and (world != 1 or args.gen == "hilbert"))
        res = None
        if want_res:
            if path is not None:
                try:
                    res = solver.residual_file(path, args.host_threads)
                except FileNotFoundError:
                    out(f"cannot open for residual {path}\n")
                    return 2
                except ValueError:
                    out(f"cannot read for residual {path}\n")
                    return 2
            else:
                res = solver.residual_generated(args.gen, args.seed)
            out(f"residual: {res:e}\n")
        elif args.residual == "compat":
            out("p == 1!\n")
        sld = None
        if args.det:  # as build/gj --det: one line after the residual line
            sld = solver.slogdet()
            sign = "nan" if sld[0] != sld[0] else f"{int(sld[0]):d}"
            out(f"slogdet: {sign} {sld[1]:.15e}\n")
        a_rows, a_gen = None, (args.gen, args.seed)
        if path is not None and (args.cond or args.rhs):  # this rank's fp64 rows, from the file again
            ids = [int(r) for r in solver.global_row_ids()]
            a_rows, a_gen = C.read_matrix_rows(path, n, ids, args.host_threads), None
        kappa = None
        if args.cond:  # as build/gj --cond: after the residual line and the slogdet line
            kappa = [solver.cond(p, A_rows=a_rows, gen=a_gen) for p in (1, float("inf"))]
            out(f"cond: {kappa[0]:e} {kappa[1]:e}\n")
        infos = None
        if args.rhs:
            x, infos = solver.solve_rhs(_rhs_block(args.rhs, n, args.nrhs, args.seed), A_rows=a_rows, gen=a_gen,
                                        trans=args.trans, bounds=args.bounds, precise=args.precise)
            worst = 0.0
            for c in infos:  # the maximum over the columns, NaN kept
                worst = c["residual"] if c["residual"] != c["residual"] or c["residual"] > worst else worst
            out("solution x:\n" + "".join(f"{v:.2f}\t" for v in x.reshape(n, -1)[:nm, 0]) +
                f"\n{'ATx-b' if args.trans else 'Ax-b'} residual: {worst:e}\n")
        if args.json and rank == 0:
            rec = {"n": n, "m": m, "ranks": world, "device": "gpu" if gpu else "cpu",
                   "dtype": args.dtype, "status": st["status"], "glob_time": glob,
                   "gflops_nominal": 2.0 * n ** 3 / glob / 1e9 if glob > 0 else 0.0,
                   "residual": res, "offdiag_pivots": st["offdiag_pivots"]}
            if "equilibrate" in st:
                rec["equilibrate"] = {k: (list(v) if isinstance(v, tuple) else v) for k, v in st["equilibrate"].items()}
            if sld is not None:
                rec["slogdet"] = [v if v - v == 0 else None for v in sld]  # JSON has no NaN or Infinity
            if kappa is not None:
                rec["cond"] = {"one": kappa[0] if kappa[0] - kappa[0] == 0 else None,
                               "inf": kappa[1] if kappa[1] - kappa[1] == 0 else None}
            if infos is not None:
                rec["axb_residual"] = worst if worst - worst == 0 else None
                rec["nrhs"] = args.nrhs
                if args.bounds:
                    for key in ("ferr", "berr"):
                        rec[f"axb_{key}_cols"] = [c[key] if c[key] - c[key] == 0 else None for c in infos]
                if args.precise:
                    rec["precise"] = True
                    for key in ("dx_rel", "err_est"):
                        rec[f"axb_{key}_cols"] = [c[key] if c[key] - c[key] == 0 else None for c in infos]
            print(json.dumps(rec), file=sys.stderr, flush=True)
        return 0
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main())
