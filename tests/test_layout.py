"""Block-row-cyclic layout math vs the reference formulas (main.cpp:95-127, :521-532)."""
import itertools

import numpy as np

from mpi_jordan_crazy_acceleration_amd.parallel.layout import Layout, global_rows, last_owner, num_block_rows, rows_owned


def ref_rows_p_process(Nr, p, k):
    # main.cpp:101-116 literally
    sender = (Nr - 1) % p
    if Nr % p == 0:
        return Nr // p
    return Nr // p + 1 if k <= sender else Nr // p


def test_rows_owned_matches_reference():
    for Nr, p in itertools.product(range(1, 40), range(1, 10)):
        assert sum(rows_owned(Nr, p, k) for k in range(p)) == Nr
        for k in range(p):
            assert rows_owned(Nr, p, k) == ref_rows_p_process(Nr, p, k)


def test_last_owner_and_blocks():
    assert num_block_rows(10, 3) == 4
    assert num_block_rows(12, 3) == 4
    assert num_block_rows(10, 12) == 1
    assert last_owner(4, 3) == 0


def test_global_rows_partition():
    for n, m, p in [(10, 3, 2), (11, 4, 3), (37, 5, 4), (10, 12, 5), (64, 8, 8), (7, 1, 3)]:
        allr = np.concatenate([global_rows(n, m, p, k) for k in range(p)])
        assert sorted(allr.tolist()) == list(range(n))
        for k in range(p):
            L = Layout(n, m, p, k)
            g = global_rows(n, m, p, k)
            for i, gi in enumerate(g):
                assert L.global_row(i) == gi
                assert (gi // m) % p == k  # block row I lives on rank I mod p


def test_real_rows_matches_brute_force():
    # n a multiple of m, a short last block row on rank 0 and on another rank, ranks that own no
    # block (p > Nr), m > n
    from mpi_jordan_crazy_acceleration_amd import load_native

    C = load_native()
    for n, m, p in itertools.product([1, 7, 64, 65, 100], [4, 16, 64], [1, 2, 3, 5]):
        for k in range(p):
            L = Layout(n, m, p, k)
            brute = sum(1 for i in range(L.nblk * m) if L.global_row(i) < n)
            assert C.layout_real_rows(n, m, p, k) == brute, (n, m, p, k)
    for n, m, p in [(64, 16, 1), (65, 16, 1), (7, 64, 1), (100, 16, 3), (65, 4, 5), (7, 4, 5)]:
        comm = C.self_comm() if p == 1 else C.shadow_comm(p, 50.0, 20.0, 16)
        lay = C.Engine(C.host_device(1), comm, n, m, "fp64").layout
        assert (lay["p"], lay["k"]) == (p, 0)
        assert lay["real_rows"] == C.layout_real_rows(n, m, p, 0) == len(global_rows(n, m, p, 0))
