"""The numpy yardstick of the partitioned solve (tests/solve_ref_dist.py) against the global one (tests/solve_ref.py): the same
x within the solve inequality, the same number of iterations, and the property the overlap of exchange and operator rests on
(no row of an interior node reads a ghost).  The partitions are those of partition_rcb / build_local; their sizes are
written down here, since the GPU tests choose their shapes by them (interior bounds that are no multiple of the 16 / 32 nodes
of an SpMV workgroup, a rank with an empty interior and fewer rows than one workgroup)."""
import numpy as np
import pytest

import solve_ref
import solve_ref_dist
import solve_systems

from solve_ref_dist import CASES, global_system, ranks_of

# (owned, interior, ghost) nodes per rank
SIZES = {("pihna_kuhn", 2): ([405, 324], [324, 243], [81, 81]),
         ("pihna_kuhn", 3): ([323, 226, 180], [242, 145, 108], [81, 90, 90]),
         ("hcc_hex", 2): ([196, 147], [147, 98], [49, 49]),
         ("pihna_kuhn3", 3): ([32, 24, 8], [16, 8, 0], None)}

@pytest.mark.parametrize("name,world", list(SIZES))
def test_partition_sizes_and_interior_rows(oracle, name, world):
    s = solve_ref_dist.case(name)
    ranks = ranks_of(name, world, oracle)
    owned, interior, ghost = SIZES[(name, world)]
    assert [rk.lp.n_owned for rk in ranks] == owned
    assert [rk.lp.n_interior for rk in ranks] == interior
    if ghost is not None:
        assert [rk.lp.xyz.shape[0] - rk.lp.n_owned for rk in ranks] == ghost
    assert all(n % 16 for n in interior if n > 16)
    for rk in ranks:
        assert solve_ref_dist.interior_rows_read_no_ghost(rk, s.nv), rk.lp.rank
        # ... and the bound is tight: the first node behind it does read one (a plan with one more interior node is refused)
        if rk.lp.n_interior < rk.lp.n_owned:
            A = rk.A.tocsr()
            row = A.indices[A.indptr[rk.lp.n_interior * s.nv]:A.indptr[rk.lp.n_interior * s.nv + 1]]
            assert row.max() >= rk.lp.n_owned * s.nv


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_partitioned_yardstick_equals_global(oracle, name, world):
    s, A, b = global_system(name, oracle)
    ranks = ranks_of(name, world, oracle)
    n_node = s.xyz.shape[0]
    for rel_tol in (1e-8, 1e-10):
        x0s = [np.zeros(rk.A.shape[1]) for rk in ranks]
        xs, info = solve_ref_dist.bicgstab_dist(ranks, x0s, rel_tol, precond=2, nv=s.nv)
        x = solve_ref_dist.gather(ranks, xs, s.nv, n_node)
        xg, ref = solve_ref_dist.yardstick(name, oracle, rel_tol)
        f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
        print(f"{s.name} world {world} tol {rel_tol:g}: iterations partitioned {info['iterations']} (restarts {info['restarts']}), global "
              f"{ref['iterations']}; residual {f['residual_norm']:.3e} <= {f['bound']:.3e}; |x - x_global| / |x_global| "
              f"{np.linalg.norm(x - xg) / np.linalg.norm(xg):.2e}")
        assert info["reason"] == solve_ref.CONVERGED
        assert abs(info["iterations"] - ref["iterations"]) <= 2
        assert abs(info["rhs_norm"] - ref["rhs_norm"]) <= 1e-13 * ref["rhs_norm"]
        # the ghost tails hold the owners' values of the returned x
        want = [v.copy() for v in xs]
        solve_ref_dist.exchange(ranks, want, s.nv)
        assert all(a.tobytes() == w.tobytes() for a, w in zip(xs, want))


def test_zero_rhs_on_one_rank_is_not_a_local_decision(oracle):
    """a rank whose own ||D^-1 b|| is 0 iterates with the others: only the global norm decides"""
    s, A, b = global_system("pihna_kuhn3", oracle)
    ranks = [solve_ref_dist.Rank(rk.lp, rk.system, rk.A, rk.b.copy()) for rk in ranks_of("pihna_kuhn3", 3, oracle)]
    ranks[2].b[:] = 0.0
    bg = solve_ref_dist.gather(ranks, [np.concatenate([rk.b, np.zeros(rk.A.shape[1] - rk.b.size)]) for rk in ranks], s.nv, s.xyz.shape[0])
    xs, info = solve_ref_dist.bicgstab_dist(ranks, [np.zeros(rk.A.shape[1]) for rk in ranks], 1e-10, precond=2, nv=s.nv)
    assert info["reason"] == solve_ref.CONVERGED and info["iterations"] > 0
    solve_ref.check_solution(A, bg, solve_ref_dist.gather(ranks, xs, s.nv, s.xyz.shape[0]), s.nv, 2, 1e-10)
