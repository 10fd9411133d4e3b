"""tests/solve_ref_mg.py -- the numpy restatement of the aggregation-multigrid preconditioner (precond = 3), the yardstick of
tests/test_gpu_solve_mg.py -- pinned on the CPU on the oracle-assembled systems of solve_systems.SOLVE_SYSTEMS: the residual
inequality of the block-Jacobi solve (the cycle is applied from the right, so the norm is the same), iteration counts against
solve_ref.bicgstab(precond=2) on the same system, the damping of their growth with the mesh, and the operator complexity.
The counts printed here are the record in DESIGN.md 7.2."""
import numpy as np
import pytest
import scipy.sparse as sps

import solve_ref
import solve_ref_mg
import solve_systems

MAX_COMPLEXITY = 1.35
_CACHE = {}


def _system(oracle, name, make=None):
    """(system, A, b, hierarchy, {rel_tol: block-Jacobi iterations}), computed once per system"""
    if name not in _CACHE:
        s = make() if make else solve_systems.get(name)
        rp, col, val, rhs = s.oracle_assemble(oracle)
        A = sps.csr_matrix((val, col, rp), shape=(rhs.size, rhs.size))
        _CACHE[name] = (s, A, s.rhs_scale * rhs, solve_ref_mg.Hierarchy(A, s.nv), {})
    return _CACHE[name]


def _both(oracle, name, rel_tol, make=None):
    s, A, b, H, bj = _system(oracle, name, make)
    if rel_tol not in bj:
        _, ref = solve_ref.bicgstab(A, b, np.zeros(b.size), rel_tol, precond=2, nv=s.nv, max_its=2000)
        assert ref["reason"] == solve_ref.CONVERGED
        bj[rel_tol] = ref["iterations"]
    x, info = solve_ref_mg.bicgstab(A, b, np.zeros(b.size), rel_tol, nv=s.nv, max_its=2000, hierarchy=H)
    print(f"{name} rel_tol {rel_tol:g}: block Jacobi {bj[rel_tol]} iterations, multigrid {info['iterations']} (restarts {info['restarts']}), "
          f"levels {info['levels']}, operator complexity {info['complexity']:.3f}")
    return s, A, b, x, info, bj[rel_tol]


@pytest.mark.parametrize("rel_tol", [1e-8, 1e-10])
@pytest.mark.parametrize("name", list(solve_systems.SOLVE_SYSTEMS))
def test_every_solve_system(oracle, name, rel_tol):
    s, A, b, x, info, bj = _both(oracle, name, rel_tol)
    assert info["reason"] == solve_ref_mg.CONVERGED
    f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
    assert abs(info["residual_norm"] - f["residual_norm"]) <= f["rho"]
    assert info["iterations"] <= bj
    assert info["complexity"] <= MAX_COMPLEXITY
    assert info["levels"][0] == (A.shape[0] // s.nv, sps.bsr_matrix(A, blocksize=(s.nv, s.nv)).indices.size)


def test_growth_with_the_mesh_is_damped(oracle):
    """pihna_kuhn at n = 8, 16, 24 (rel_tol 1e-8): at n = 24 the multigrid count is at most half the block-Jacobi count"""
    counts = {}
    for n in (8, 16, 24):
        s, A, b, x, info, bj = _both(oracle, f"pihna_kuhn{n}", 1e-8, make=lambda n=n: solve_systems.pihna_kuhn(n))
        assert info["reason"] == solve_ref_mg.CONVERGED
        solve_ref.check_solution(A, b, x, s.nv, 2, 1e-8)
        assert info["complexity"] <= MAX_COMPLEXITY
        counts[n] = (bj, info["iterations"])
    print("K(n): (block Jacobi, multigrid)", counts)
    assert all(mg <= bj for bj, mg in counts.values())
    assert 2 * counts[24][1] <= counts[24][0]


def test_hierarchy_properties(oracle):
    """every node in exactly one aggregate, pass-1 aggregates of at most AGG_CAP nodes, every fine block in exactly one list,
    no empty list, ascending columns -- on the hub (one node with 740 neighbours) and the unstructured hydrogel mesh"""
    for name in ("pihna_hub", "pihna_hydrogel"):
        s, A, b, H, _ = _system(oracle, name)
        bptr, bcol, _ = solve_ref_mg.block_pattern(A, s.nv)
        steps = solve_ref_mg.pattern_hierarchy(bptr, bcol)
        assert len(steps) + 1 == len(H.levels) >= 2
        for st in steps:
            n = bptr.size - 1
            assert st["agg"].min() == 0 and st["agg"].max() == st["n"] - 1 and st["agg"].size == n
            sizes = np.bincount(st["agg"], minlength=st["n"])
            assert sizes.min() >= 1 and sizes.sum() == n
            assert st["pass1_sizes"].size == st["n_pass1"] and solve_ref_mg.MIN_FREE + 1 <= st["pass1_sizes"].min()
            assert st["pass1_sizes"].max() <= solve_ref_mg.AGG_CAP
            assert np.array_equal(np.sort(st["cidx"]), np.arange(bcol.size)) and np.diff(st["cptr"]).min() >= 1
            for i in range(st["n"]):
                assert np.all(np.diff(st["bcol"][st["bptr"][i]:st["bptr"][i + 1]]) > 0)
            bptr, bcol = st["bptr"], st["bcol"]
        if name == "pihna_hub":
            assert np.diff(H.levels[0]["bptr"]).max() >= 740


def test_cycle_is_a_fixed_linear_operator(oracle):
    s, A, b, H, _ = _system(oracle, "pihna_kuhn")
    rng = np.random.default_rng(1)
    u, v = rng.standard_normal(b.size), rng.standard_normal(b.size)
    lhs, rhs = H.cycle(2.0 * u - 3.0 * v), 2.0 * H.cycle(u) - 3.0 * H.cycle(v)
    assert np.linalg.norm(lhs - rhs) <= 1e-12 * np.linalg.norm(rhs)
    assert H.cycle(u).tobytes() == H.cycle(u).tobytes()
