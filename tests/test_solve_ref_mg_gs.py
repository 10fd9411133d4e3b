"""tests/solve_ref_mg_gs.py -- the numpy restatement of the multigrid cycle with the multicolour Gauss-Seidel smoother (option
"mg_smoother" = 1), the yardstick of tests/test_gpu_solve_mg_gs.py -- pinned on the CPU on oracle-assembled systems: those of
solve_systems.SOLVE_SYSTEMS and the Kuhn meshes K(16) and K(24).  Convergence, the residual inequality of the block-Jacobi solve
(the cycle is applied from the right, so the norm is the same), iteration counts against the damped-Jacobi cycle of
solve_ref_mg.py on the same hierarchy, and the colourings.  The counts printed here are the record in DESIGN.md 7.2."""
import numpy as np
import pytest
import scipy.sparse as sps

import solve_ref
import solve_ref_mg
import solve_ref_mg_gs
import solve_systems

KUHN = {"pihna_kuhn16": 16, "pihna_kuhn24": 24}
SYSTEMS = list(solve_systems.SOLVE_SYSTEMS) + list(KUHN)
_CACHE = {}


def _system(oracle, name):
    """(system, A, b, Jacobi-smoother hierarchy, Gauss-Seidel hierarchy on the same levels), computed once per system"""
    if name not in _CACHE:
        s = solve_systems.pihna_kuhn(KUHN[name]) if name in KUHN else solve_systems.get(name)
        rp, col, val, rhs = s.oracle_assemble(oracle)
        A = sps.csr_matrix((val, col, rp), shape=(rhs.size, rhs.size))
        base = solve_ref_mg.Hierarchy(A, s.nv)
        _CACHE[name] = (s, A, s.rhs_scale * rhs, base, solve_ref_mg_gs.Hierarchy(A, s.nv, base=base))
    return _CACHE[name]


@pytest.mark.parametrize("rel_tol", [1e-8, 1e-10])
@pytest.mark.parametrize("name", SYSTEMS)
def test_gauss_seidel_smoother(oracle, name, rel_tol):
    s, A, b, base, H = _system(oracle, name)
    _, jac = solve_ref_mg.bicgstab(A, b, np.zeros(b.size), rel_tol, nv=s.nv, max_its=2000, hierarchy=base)
    x, info = solve_ref_mg_gs.bicgstab(A, b, np.zeros(b.size), rel_tol, nv=s.nv, max_its=2000, hierarchy=H)
    print(f"{name} rel_tol {rel_tol:g}: Jacobi smoother {jac['iterations']} iterations, Gauss-Seidel smoother {info['iterations']} "
          f"(restarts {info['restarts']}), colours per level {info['colours']}, levels {info['levels']}")
    assert jac["reason"] == solve_ref_mg.CONVERGED and info["reason"] == solve_ref_mg_gs.CONVERGED
    f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
    assert abs(info["residual_norm"] - f["residual_norm"]) <= f["rho"]
    assert info["iterations"] <= jac["iterations"]
    assert info["levels"] == base.level_sizes()
    if name == "pihna_kuhn24" and rel_tol == 1e-8:
        assert 4 * info["iterations"] <= 3 * jac["iterations"]


@pytest.mark.parametrize("name", SYSTEMS)
def test_colourings_are_proper(oracle, name):
    """on every level: no two coupled nodes share a colour, every node has one, the lists are the colours' nodes in ascending
    order, and greedy needs at most as many colours as the longest row has blocks"""
    s, A, b, base, H = _system(oracle, name)
    assert len(H.colours()) == len(H.levels)
    for lv, k in zip(H.levels, H.colours()):
        bptr, bcol, col, cptr, nodes = lv["bptr"], lv["bcol"], lv["colour"], lv["cptr"], lv["cnodes"]
        assert solve_ref_mg_gs.is_proper(bptr, bcol, col)
        assert col.min() == 0 and col.max() == k - 1 and 1 <= k <= np.diff(bptr).max()
        assert cptr[0] == 0 and cptr[-1] == lv["n"] and np.diff(cptr).min() >= 1
        np.testing.assert_array_equal(np.sort(nodes), np.arange(lv["n"]))
        for c in range(k):
            mine = nodes[cptr[c]:cptr[c + 1]]
            assert np.all(col[mine] == c) and np.all(np.diff(mine) > 0)
    if name == "pihna_hub":   # the node with 739 neighbours shares its colour with nodes outside its row only; 9 colours do
        lv = H.levels[0]
        hub = int(np.argmax(np.diff(lv["bptr"])))
        row = lv["bcol"][lv["bptr"][hub]:lv["bptr"][hub + 1]]
        assert row.size >= 740 and H.colours()[0] < 16
        assert np.count_nonzero(lv["colour"][row] == lv["colour"][hub]) == 1     # itself


def test_the_first_sweep_keeps_its_damping_and_the_rest_is_undamped(oracle):
    """one cycle on a two-level cut of the algorithm, written out: x1 = w r, coarse correction, then one forward sweep"""
    s, A, b, base, H = _system(oracle, "pihna_kuhn")
    r = np.random.default_rng(3).standard_normal(b.size)
    lv = H.levels[0]
    x = H.omega * r
    P = lv["P"]
    x = x + P @ H.cycle(P.T @ (r - H._op(0, x)), 1)
    Ah = (H.M0 @ H.A0).tocsr()
    for c in range(lv["cptr"].size - 1):     # Gauss-Seidel on D^-1 A, node blocks of one colour at a time
        nodes = lv["cnodes"][lv["cptr"][c]:lv["cptr"][c + 1]].astype(np.int64)
        dofs = (nodes[:, None] * s.nv + np.arange(s.nv)[None]).reshape(-1)
        x[dofs] += r[dofs] - Ah[dofs] @ x
    got = H.cycle(r)
    assert np.linalg.norm(got - x) <= 1e-12 * np.linalg.norm(x)
    assert H.cycle(r).tobytes() == got.tobytes()
