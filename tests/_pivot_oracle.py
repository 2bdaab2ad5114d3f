"""The pivot sequences the engine tests pin (test_gpu_engine.py, test_host_engine.py): the numpy oracle's
sequence per (n, m, seed), computed once.  Without exact ties the sequence depends on neither the rank
count nor the panel depth, so one oracle run serves every schedule of a shape."""
import functools

from mpi_jordan_crazy_acceleration_amd.utils import gauss_jordan_reference, generate_matrix, physical_pivots

SEED = 21
SHAPES = [(96, 16), (250, 37), (480, 60), (700, 100), (896, 128), (1100, 200), (1500, 300)]
MIN_GAP = 1e-3  # best against second-best score, relative: far above the rounding of an fp64 score


def matrix(n):
    """Reversed rows of the seeded random matrix: weak diagonal blocks, so pivots leave the diagonal."""
    return generate_matrix(n, "random", SEED)[::-1].copy()


@functools.lru_cache(maxsize=None)
def oracle(n, m):
    """(inverse, physical pivot sequence) of matrix(n) at block size m; asserts, on the oracle alone,
    that every step's winner is clear of the runner-up and that the case exercises off-diagonal pivots."""
    inv, piv, gaps = gauss_jordan_reference(matrix(n), m, 1, return_gaps=True)
    assert min(gaps) >= MIN_GAP, (n, m, gaps)
    phys = physical_pivots(piv)
    assert sum(1 for t, s in enumerate(phys) if s != t) >= 5, phys
    inv.setflags(write=False)
    return inv, phys


def grid_cases():
    """(n, m, p, depth, comm): every shape at p = 1 and 3, depth 2; two shapes over p x depth and on the
    asynchronous loopback transport."""
    cases = [(n, m, p, 2, "loopback") for n, m in SHAPES for p in (1, 3)]
    for n, m in [(480, 60), (896, 128)]:
        cases += [(n, m, p, d, "loopback") for p in (1, 2, 3, 4) for d in (1, 2, 4)]
        cases.append((n, m, 3, 2, "async"))
    return sorted(set(cases))


def case_id(c):
    n, m, p, depth, comm = c
    return f"n{n}-m{m}-p{p}-d{depth}-{comm}"
