"""tests/solve_ref_ilu_dist.py -- the numpy yardstick of the rank-local block ILU(0) (RDC_PRECOND_ILU0_LOCAL), what
tests/test_gpu_solve_ilu_dist.py holds the device to -- pinned on the CPU: iteration counts from x0 = 0 at 1e-8 and 1e-10 for one,
two and three ranks on the systems of solve_ref_dist.CASES, the residual inequality of the block-Jacobi solve on the gathered x
(M comes from the right, so the norm is the same), world 1 = the single-partition ILU(0) of tests/test_solve_ref_ilu.py, and every
world above 1 still beats block Jacobi.  The counts are the record in DESIGN.md 7.4."""
import numpy as np
import pytest

import solve_ref
import solve_ref_dist
import solve_ref_ilu
import solve_ref_ilu_dist
from test_solve_ref_ilu import PINNED as PINNED_ONE

TOLS = (1e-8, 1e-10)
#           (system, ranks): iterations at 1e-8, at 1e-10
PINNED = {("pihna_kuhn", 1): (9, 11), ("pihna_kuhn", 2): (10, 12), ("pihna_kuhn", 3): (10, 13),
          ("hcc_hex", 1): (5, 6), ("hcc_hex", 2): (7, 9), ("hcc_hex", 3): (8, 10),
          ("pihna_kuhn3", 1): (4, 5), ("pihna_kuhn3", 2): (6, 7), ("pihna_kuhn3", 3): (5, 7)}


@pytest.mark.parametrize("name,world", list(PINNED))
def test_iteration_counts(oracle, name, world):
    s, A, b = solve_ref_dist.global_system(name, oracle)
    for rel_tol, want in zip(TOLS, PINNED[(name, world)]):
        x, info = solve_ref_ilu_dist.yardstick(name, world, oracle, rel_tol)
        jac = solve_ref_dist.yardstick(name, oracle, rel_tol)[1]
        f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
        print(f"{name} world {world} tol {rel_tol:g}: {info['iterations']} iterations (restarts {info['restarts']}), block Jacobi "
              f"{jac['iterations']}; residual {f['residual_norm']:.3e} <= {f['bound']:.3e}")
        assert info["reason"] == solve_ref.CONVERGED and info["restarts"] == 0
        assert abs(info["residual_norm"] - f["residual_norm"]) <= f["rho"]
        assert info["iterations"] == want
        if world > 1:
            assert info["iterations"] < jac["iterations"]


@pytest.mark.parametrize("name", ["pihna_kuhn", "hcc_hex"])
def test_one_rank_is_the_single_partition_ilu(oracle, name):
    """one rank owns every node in the global order: the owned square is the matrix, the counts are those of test_solve_ref_ilu.py
    and the x is that of solve_ref_ilu.bicgstab up to the rounding of the rank's own assembly"""
    s, A, b = solve_ref_dist.global_system(name, oracle)
    rk, = solve_ref_dist.ranks_of(name, 1, oracle)
    assert rk.lp.n_owned == s.xyz.shape[0] == rk.A.shape[1] // s.nv
    assert PINNED[(name, 1)] == PINNED_ONE[name][:2]
    for rel_tol in TOLS:
        x, info = solve_ref_ilu_dist.yardstick(name, 1, oracle, rel_tol)
        xg, ref = solve_ref_ilu.bicgstab(A, b, np.zeros(b.size), rel_tol, nv=s.nv, max_its=2000)
        assert info["iterations"] == ref["iterations"]
        assert np.linalg.norm(x - xg) <= 10.0 * rel_tol * np.linalg.norm(xg)


def test_the_factor_is_that_of_the_owned_square_and_needs_no_ghost(oracle):
    """a rank's M reads and writes owned entries only, and dropping the couplings across ranks makes it another operator than the
    global factor restricted to the rank's rows"""
    name, world = "pihna_kuhn", 2
    s, A, b = solve_ref_dist.global_system(name, oracle)
    ranks = solve_ref_dist.ranks_of(name, world, oracle)
    fs = solve_ref_ilu_dist.factors(ranks, s.nv)
    glob = solve_ref_ilu.Factor(A, s.nv)
    y = np.random.default_rng(4).standard_normal(b.size)
    zg = glob.apply(y).reshape(-1, s.nv)
    for rk, f in zip(ranks, fs):
        assert f.n == rk.lp.n_owned and f.singular == 0
        assert int(f.bcol.max()) < rk.lp.n_owned
        mine = rk.lp.node_global[:rk.lp.n_owned]
        z = f.apply(y.reshape(-1, s.nv)[mine].reshape(-1))
        assert z.size == rk.lp.n_owned * s.nv and np.all(np.isfinite(z))
        assert np.abs(z - zg[mine].reshape(-1)).max() > 1e-6 * np.abs(z).max()
