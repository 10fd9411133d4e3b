"""tests/solve_ref.py -- the numpy restatement of rdc_solve's algorithm that the GPU tests use as the yardstick for
iteration counts -- pinned on the CPU on oracle-assembled systems: by the residual inequality of the GPU solve test
(solve_ref.check_solution), and for the HCC system against scipy's direct solve.

RIPF: the solver case takes its time step from the state (cell Courant number 1 of the fb transport,
solve_systems.ripf_tet); at the shipped time_step 0.1 on the synthetic state (Courant number about 900) the operator is
indefinite (K(6): 30 of 1029 eigenvalues of D^-1 A have a negative real part) and BiCGStab with a Jacobi-class
preconditioner stagnates: test_ripf_at_courant_900_reports_non_convergence pins that the algorithm then says so."""
import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spl

import solve_ref
import solve_systems


def _system(oracle, name):
    s = solve_systems.get(name)
    rp, col, val, rhs = s.oracle_assemble(oracle)
    return s, sps.csr_matrix((val, col, rp), shape=(rhs.size, rhs.size)), s.rhs_scale * rhs


@pytest.mark.parametrize("rel_tol", [1e-8, 1e-10])
@pytest.mark.parametrize("name", ["pihna_kuhn", "ripf_tet", "hcc_tet", "hcc_hex", "solid_cube"])
def test_residual_inequality(oracle, name, rel_tol):
    s, A, b = _system(oracle, name)
    x, info = solve_ref.bicgstab(A, b, np.zeros(b.size), rel_tol, precond=2, nv=s.nv, max_its=2000)
    print(name, rel_tol, info)
    assert info["reason"] == solve_ref.CONVERGED
    f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
    assert abs(info["residual_norm"] - f["residual_norm"]) <= f["rho"]


@pytest.mark.parametrize("precond", [0, 1, 2])
def test_three_preconditioners_on_pihna(oracle, precond):
    s, A, b = _system(oracle, "pihna_kuhn")
    x, info = solve_ref.bicgstab(A, b, np.zeros(b.size), 1e-10, precond=precond, nv=5, max_its=5000)
    assert info["reason"] == solve_ref.CONVERGED
    solve_ref.check_solution(A, b, x, 5, precond, 1e-10)


def test_hcc_against_direct_solve(oracle):
    s, A, b = _system(oracle, "hcc_hex")
    x, info = solve_ref.bicgstab(A, b, np.zeros(b.size), 1e-13, precond=2, nv=3, max_its=2000)
    assert info["reason"] == solve_ref.CONVERGED
    x0 = spl.spsolve(A.tocsc(), b)
    assert np.linalg.norm(x - x0) <= 1e-11 * np.linalg.norm(x0)


def test_ripf_at_courant_900_reports_non_convergence(oracle):
    s, A, b = _system(oracle, "ripf_tet_dt01")
    x, info = solve_ref.bicgstab(A, b, np.zeros(b.size), 1e-8, precond=2, nv=3, max_its=300)
    M, _, _ = solve_ref.precond_inverse(A, 3, 2)
    true = float(np.linalg.norm(M @ (b - A @ x)))
    print(info, true)
    assert info["reason"] == solve_ref.MAX_ITS and np.all(np.isfinite(x))
    # why: the fb rows have negative diagonal entries and the preconditioned operator is indefinite
    ev = np.linalg.eigvals((M @ A).toarray())
    print("eigenvalues of D^-1 A with a negative real part:", int((ev.real < 0).sum()), "of", ev.size,
          "; smallest fb diagonal entry", A.diagonal()[2::3].min())
    assert A.diagonal()[2::3].min() < 0.0 and int((ev.real < 0).sum()) == 30 and ev.size == 1029
    assert abs(info["residual_norm"] - true) <= 1e-10 * true and true > 1e-8 * info["rhs_norm"]


def test_outcomes(oracle):
    s, A, b = _system(oracle, "pihna_kuhn")
    x, info = solve_ref.bicgstab(A, np.zeros(b.size), np.ones(b.size), 1e-10, precond=2, nv=5)
    assert info["reason"] == solve_ref.CONVERGED and info["iterations"] == 0 and not x.any()
    x, info = solve_ref.bicgstab(A, b, np.zeros(b.size), 1e-10, precond=2, nv=5, max_its=1)
    assert info["reason"] == solve_ref.MAX_ITS and info["iterations"] == 1 and np.all(np.isfinite(x))
    bn = b.copy()
    bn[7] = np.nan
    x, info = solve_ref.bicgstab(A, bn, np.zeros(b.size), 1e-10, precond=2, nv=5)
    assert info["reason"] == solve_ref.NOT_FINITE and not x.any()
