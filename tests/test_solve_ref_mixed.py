"""tests/solve_ref_mixed.py -- the numpy restatement of rdc_solve_mixed, yardstick for the iteration counts of the mixed
GPU tests -- pinned on the CPU on oracle-assembled systems.  The returned x is held to the UNCHANGED fp64 inequality of
solve_ref.check_solution: iterating on fl32(D^-1 A) changes the path, never what "converged" means, because every
claim of the recurrence is confirmed on the fp64 residual.  At rel_tol 1e-8 the iteration count may not exceed
1.5 x that of the fp64 algorithm + 2; at 1e-10 the ratio is printed only (the hydrogel mesh sits near 1.9)."""
import numpy as np
import pytest
import scipy.sparse as sps

import solve_ref
import solve_ref_mixed
import solve_systems

SYSTEMS = ["pihna_kuhn", "ripf_tet", "hcc_tet", "hcc_hex", "solid_cube", "pihna_hub", "pihna_hydrogel"]


def _system(oracle, name):
    s = solve_systems.get(name)
    rp, col, val, rhs = s.oracle_assemble(oracle)
    return s, sps.csr_matrix((val, col, rp), shape=(rhs.size, rhs.size)), s.rhs_scale * rhs


@pytest.mark.parametrize("rel_tol", [1e-8, 1e-10])
@pytest.mark.parametrize("name", SYSTEMS)
def test_mixed_yardstick(oracle, name, rel_tol):
    s, A, b = _system(oracle, name)
    x, info = solve_ref_mixed.bicgstab(A, b, np.zeros(b.size), rel_tol, precond=2, nv=s.nv, max_its=2000)
    _, ref = solve_ref.bicgstab(A, b, np.zeros(b.size), rel_tol, precond=2, nv=s.nv, max_its=2000)
    S = solve_ref_mixed.scaled_f32(A, s.nv, 2)
    nz = np.abs(S.data[S.data != 0.0])
    print(f"{name} rel_tol {rel_tol:g}: iterations fp64 {ref['iterations']} -> mixed {info['iterations']} "
          f"(ratio {info['iterations'] / max(ref['iterations'], 1):.2f}), restarts {ref['restarts']} -> {info['restarts']}; "
          f"|fl32(D^-1 A)| in [{nz.min():.1e}, {nz.max():.1e}]")
    assert info["reason"] == solve_ref.CONVERGED and ref["reason"] == solve_ref.CONVERGED
    f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
    assert abs(info["residual_norm"] - f["residual_norm"]) <= f["rho"]
    assert np.all(np.isfinite(S.data))
    if rel_tol == 1e-8:
        assert info["iterations"] <= 1.5 * ref["iterations"] + 2, (info, ref)


def test_ripf_at_courant_900_still_reports_non_convergence(oracle):
    s, A, b = _system(oracle, "ripf_tet_dt01")
    x, info = solve_ref_mixed.bicgstab(A, b, np.zeros(b.size), 1e-8, precond=2, nv=3, max_its=300)
    M, _, _ = solve_ref.precond_inverse(A, 3, 2)
    true = float(np.linalg.norm(M @ (b - A @ x)))
    print(info, true)
    assert info["reason"] == solve_ref.MAX_ITS and info["iterations"] == 300 and np.all(np.isfinite(x))
    assert abs(info["residual_norm"] - true) <= 1e-10 * true and true > 1e-8 * info["rhs_norm"]


def test_returns_what_solve_ref_returns(oracle):
    s, A, b = _system(oracle, "hcc_tet")
    x, info = solve_ref_mixed.bicgstab(A, np.zeros(b.size), np.ones(b.size), 1e-10, precond=2, nv=3)
    assert info["reason"] == solve_ref.CONVERGED and info["iterations"] == 0 and not x.any()
    x, info = solve_ref_mixed.bicgstab(A, b, np.zeros(b.size), 1e-10, precond=2, nv=3, max_its=1)
    _, ref = solve_ref.bicgstab(A, b, np.zeros(b.size), 1e-10, precond=2, nv=3, max_its=1)
    assert set(info) == set(ref) and info["reason"] == solve_ref.MAX_ITS and info["iterations"] == 1
