"""tests/solve_ref_gmres.py -- the numpy restatement of the GMRES path of rdc_solve, the yardstick of tests/test_gpu_solve_gmres.py --
pinned on the CPU on oracle-assembled systems: the residual inequality of the solver tests, a direct solve, the comparison with
BiCGStab that motivates the method (Arnoldi steps <= 2 x BiCGStab iterations = operator applications, on every system and
preconditioner where GMRES(m) converges), and the record of where GMRES(30) does not converge."""
import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import solve_ref
import solve_ref_gmres
import solve_ref_ilu
import solve_ref_mg
import solve_systems

_CACHE = {}
TOLS = (1e-8, 1e-10)
# (system, precond, restart): the rows of the comparison that converge; hydrogel with precond 3 is 59 against 60
# operator applications, too close to pin
ROWS = [("pihna_kuhn", 2, 30), ("pihna_kuhn", 3, 30), ("pihna_kuhn", 4, 30), ("pihna_kuhn16", 3, 30), ("pihna_kuhn16", 4, 30),
        ("hcc_hex", 2, 30), ("hcc_hex", 3, 30), ("hcc_hex", 4, 30), ("solid_cube", 2, 30), ("solid_cube", 3, 30), ("solid_cube", 4, 30),
        ("ripf_tet", 2, 30), ("ripf_tet", 4, 30), ("pihna_hub", 2, 30), ("pihna_hub", 4, 30), ("pihna_hydrogel", 4, 60)]


def _system(oracle, name):
    if name not in _CACHE:
        s = solve_systems.pihna_kuhn(16) if name == "pihna_kuhn16" else solve_systems.get(name)
        rp, col, val, rhs = s.oracle_assemble(oracle)
        A = sps.csr_matrix((val, col, rp), shape=(rhs.size, rhs.size))
        _CACHE[name] = dict(s=s, A=A, b=s.rhs_scale * rhs, right={})
    return _CACHE[name]


def _right(S, precond):
    """the right preconditioner of `precond` on block Jacobi's system (None for 0, 1, 2), built once per system"""
    if precond not in S["right"]:
        S["right"][precond] = {3: lambda: solve_ref_mg.Hierarchy(S["A"], S["s"].nv).cycle,
                               4: lambda: solve_ref_ilu.Factor(S["A"], S["s"].nv).apply}.get(precond, lambda: None)()
    return S["right"][precond]


def _both(S, precond, rel_tol, restart, max_its=600):
    A, b, nv, right = S["A"], S["b"], S["s"].nv, _right(S, precond)
    x0 = np.zeros(b.size)
    xg, g = solve_ref_gmres.gmres(A, b, x0, rel_tol, max_its=max_its, precond=min(precond, 2), nv=nv, right=right, restart=restart)
    xb, bi = solve_ref.bicgstab(A, b, x0, rel_tol, max_its=max_its, precond=min(precond, 2), nv=nv, right=right)
    return xg, g, xb, bi


@pytest.mark.parametrize("rel_tol", TOLS)
@pytest.mark.parametrize("name", ["pihna_kuhn", "ripf_tet", "hcc_tet", "hcc_hex", "solid_cube"])
def test_residual_inequality(oracle, name, rel_tol):
    S = _system(oracle, name)
    x, info = solve_ref_gmres.gmres(S["A"], S["b"], np.zeros(S["b"].size), rel_tol, max_its=600, precond=2, nv=S["s"].nv)
    assert info["reason"] == solve_ref_gmres.CONVERGED, info
    f = solve_ref.check_solution(S["A"], S["b"], x, S["s"].nv, 2, rel_tol)
    assert abs(info["residual_norm"] - f["residual_norm"]) <= f["rho"]
    assert info["restarts"] == info["cycles"] - 1 == (info["iterations"] - 1) // 30


def test_against_a_direct_solve(oracle):
    S = _system(oracle, "hcc_hex")
    x, info = solve_ref_gmres.gmres(S["A"], S["b"], np.zeros(S["b"].size), 1e-12, max_its=600, precond=2, nv=S["s"].nv)
    want = spla.spsolve(S["A"].tocsc(), S["b"])
    assert info["reason"] == solve_ref_gmres.CONVERGED
    M, _, cond = solve_ref.precond_inverse(S["A"], S["s"].nv, 2)
    kappa = np.linalg.cond((M @ S["A"]).toarray())
    assert np.linalg.norm(x - want) <= kappa * 1e-12 * np.linalg.norm(want) + 1e-13 * np.linalg.norm(want), (kappa, np.linalg.norm(x - want))


@pytest.mark.parametrize("name,precond,restart", ROWS)
def test_fewer_operator_applications_than_bicgstab(oracle, name, precond, restart):
    S = _system(oracle, name)
    xg, g, xb, bi = _both(S, precond, 1e-8, restart)
    print(f"{name} precond {precond} restart {restart}: BiCGStab 2 x {bi['iterations']} = {2 * bi['iterations']} applications, "
          f"GMRES {g['iterations']} steps in {g['cycles']} cycles")
    assert g["reason"] == solve_ref_gmres.CONVERGED and bi["reason"] == solve_ref.CONVERGED, (g, bi)
    solve_ref.check_solution(S["A"], S["b"], xg, S["s"].nv, 2, 1e-8)
    assert g["iterations"] <= 2 * bi["iterations"], (g, bi)


def test_hydrogel_block_jacobi_stagnates_and_says_so(oracle):
    """GMRES(30) on block Jacobi's system of the hydrogel mesh does not converge (it stagnates near 6.6e-7 relative, at every
    restart length tried up to 100): the solve ends at max_its with the true residual of the x it returns"""
    S = _system(oracle, "pihna_hydrogel")
    A, b, nv = S["A"], S["b"], S["s"].nv
    x, info = solve_ref_gmres.gmres(A, b, np.zeros(b.size), 1e-8, max_its=300, precond=2, nv=nv, restart=30)
    M, _, _ = solve_ref.precond_inverse(A, nv, 2)
    rn = float(np.linalg.norm(M @ (b - A @ x)))
    print(f"hydrogel precond 2 restart 30: {info['iterations']} steps, {info['restarts']} restarts, residual {rn / info['rhs_norm']:.2e} relative")
    assert info["reason"] == solve_ref_gmres.MAX_ITS and info["iterations"] == 300 and info["restarts"] == 9
    assert info["residual_norm"] == rn and rn > 1e-8 * info["rhs_norm"]


def test_arnoldi_in_extended_precision(oracle):
    """the form the device hook is held to: the relation A V_k = V_{k+1} H and the orthogonality, to extended precision"""
    S = _system(oracle, "ripf_tet")
    M, _, _ = solve_ref.precond_inverse(S["A"], S["s"].nv, 2)
    Op = (M @ S["A"]).astype(np.longdouble).toarray()
    V, H, done = solve_ref_gmres.arnoldi(lambda v: Op @ v, S["b"], 12, refine=True, dtype=np.longdouble)
    assert done == 12 and V.dtype == np.longdouble
    assert np.abs(V @ V.T - np.eye(13)).max() <= 1e-15
    assert np.abs(Op @ V[:12].T - V.T @ H).max() <= 1e-15 * np.abs(H).max()
