"""tests/solve_ref_ilu.py -- the numpy restatement of the multicolour block ILU(0) preconditioner (RDC_PRECOND_ILU0), the
yardstick of tests/test_gpu_solve_ilu.py -- pinned on the CPU on oracle-assembled systems of solve_systems: iteration counts from
x0 = 0 at 1e-8 and 1e-10, the residual inequality of the block-Jacobi solve (M is applied from the right, so the norm is the same),
exactness where ILU(0) is exact, and the case it does not fix.  The counts are the record in DESIGN.md 7.4.

pihna_hydrogel at 1e-10: 48 here.  Its diagonal blocks have condition numbers up to 2e13 and the FP64 factor differs from the
extended-precision one by 5e-11 (2-norm) to 6e-10 (largest entry), which is the size of the tolerance: the count moves with the
rounding of the factor -- 48 with the FP64 factor in either sum order of the apply, 50 with the extended-precision factor."""
import numpy as np
import pytest
import scipy.sparse as sps

import solve_ref
import solve_ref_ilu
import solve_systems

#           system: (iterations at 1e-8, at 1e-10, colours)
PINNED = {"pihna_kuhn": (9, 11, 10), "pihna_hydrogel": (47, 48, 10), "hcc_hex": (5, 6, 15), "ripf_tet": (5, 6, 9), "solid_cube": (18, 21, 8)}
_CACHE = {}


def _system(oracle, name):
    if name not in _CACHE:
        s = solve_systems.get(name)
        rp, col, val, rhs = s.oracle_assemble(oracle)
        A = sps.csr_matrix((val, col, rp), shape=(rhs.size, rhs.size))
        _CACHE[name] = (s, A, s.rhs_scale * rhs, solve_ref_ilu.Factor(A, s.nv))
    return _CACHE[name]


@pytest.mark.parametrize("name", list(PINNED))
def test_iteration_counts(oracle, name):
    s, A, b, f = _system(oracle, name)
    assert f.singular == 0 and int(f.colour.max()) + 1 == PINNED[name][2]
    for rel_tol, want in zip((1e-8, 1e-10), PINNED[name]):
        x, info = solve_ref_ilu.bicgstab(A, b, np.zeros(b.size), rel_tol, nv=s.nv, max_its=2000, factor=f)
        print(f"{name} rel_tol {rel_tol:g}: {info['iterations']} iterations (restarts {info['restarts']}), {info['colours']} colours")
        assert info["reason"] == solve_ref_ilu.CONVERGED
        fig = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
        assert abs(info["residual_norm"] - fig["residual_norm"]) <= fig["rho"]
        assert info["iterations"] == want


def test_the_two_forms_of_the_apply_agree(oracle):
    """colour after colour on sparse rows (what bicgstab runs) against node after node: the order of a row's sum only"""
    s, A, b, f = _system(oracle, "pihna_kuhn")
    y = np.random.default_rng(11).standard_normal(b.size)
    z = f.apply(y)
    g = solve_ref_ilu.Factor.__new__(solve_ref_ilu.Factor)
    g.__dict__.update(f.__dict__)
    g.cptr = None
    assert np.abs(g.apply(y) - z).max() <= 64 * np.finfo(np.float64).eps * np.abs(z).max()
    # it IS a preconditioner: M A^ is much closer to the identity than A^ is
    Ah = solve_ref.precond_inverse(A, s.nv, 2)[0] @ A
    assert np.linalg.norm(f.apply(Ah @ y) - y) < 0.5 * np.linalg.norm(Ah @ y - y)


def _block_tridiagonal(n, nv, seed):
    rng = np.random.default_rng(seed)
    rows, cols, data = [], [], []
    for i in range(n):
        for j in (i - 1, i, i + 1):
            if 0 <= j < n:
                blk = rng.standard_normal((nv, nv)) + (4.0 * nv * np.eye(nv) if i == j else 0.0)
                for a in range(nv):
                    for c in range(nv):
                        rows.append(i * nv + a); cols.append(j * nv + c); data.append(blk[a, c])
    return sps.csr_matrix((data, (rows, cols)), shape=(n * nv, n * nv))


def _dense_lu(f):
    """(L, U) of a Factor as dense matrices in the numbering of the matrix (L with its identity diagonal)"""
    nv, n = f.nv, f.n
    L, U = np.eye(n * nv), np.zeros((n * nv, n * nv))
    for i in range(n):
        for kb in f.lower[i]:
            L[i * nv:(i + 1) * nv, f.bcol[kb] * nv:(f.bcol[kb] + 1) * nv] = f.F[kb]
        for kb in list(f.upper[i]) + [f.diag[i]]:
            U[i * nv:(i + 1) * nv, f.bcol[kb] * nv:(f.bcol[kb] + 1) * nv] = f.F[kb]
    return L, U


def _arrow(n, nv, seed):
    """n - 1 nodes coupled to the last one only"""
    rng = np.random.default_rng(seed)
    A = np.zeros((n * nv, n * nv))
    for i in range(n):
        for j in {i, n - 1} | (set(range(n)) if i == n - 1 else set()):
            A[i * nv:(i + 1) * nv, j * nv:(j + 1) * nv] = rng.standard_normal((nv, nv)) + (4.0 * nv * np.eye(nv) if i == j else 0.0)
    return sps.csr_matrix(A)


@pytest.mark.parametrize("order", ["colour", "natural"])
@pytest.mark.parametrize("nv", [1, 3, 5])
def test_factor_and_apply_on_a_block_tridiagonal_matrix(order, nv):
    """In both orders: the apply solves with the factor, (LU) (M y) = y, and LU equals A^ on the pattern, which defines ILU(0).
    In the natural order eliminating a node of a chain fills nothing, so ILU(0) is the LU factorisation and M A^ x = x to 1e-12.
    In the colour order (red-black on a chain) that does NOT hold: eliminating an interior node of the first colour couples its two
    neighbours, a block the pattern lacks and ILU(0) drops.  The colour order is exact where no such block arises: on an arrow
    matrix whose hub comes last, the leaves are the first colour and fill nothing."""
    A = _block_tridiagonal(37, nv, 5 + nv)
    f = solve_ref_ilu.Factor(A, nv, order=order)
    Ah = (solve_ref.precond_inverse(A, nv, 2)[0] @ A).toarray()
    L, U = _dense_lu(f)
    x = np.random.default_rng(7).standard_normal(A.shape[0])
    assert np.abs(L @ (U @ f.apply(x)) - x).max() <= 1e-12 * np.abs(x).max()
    on = np.kron((np.abs(sps.csr_matrix(A).toarray()).reshape(37, nv, 37, nv).sum(axis=(1, 3)) > 0), np.ones((nv, nv))) > 0
    assert np.abs((L @ U - Ah)[on]).max() <= 1e-12 * np.abs(Ah).max()
    if order == "natural":
        assert np.abs(f.apply(Ah @ x) - x).max() <= 1e-12 * np.abs(x).max()
    else:
        assert int(f.colour.max()) + 1 == 2
        B = _arrow(23, nv, 9 + nv)
        g = solve_ref_ilu.Factor(B, nv)
        assert g.colour.tolist() == [0] * 22 + [1]
        Bh = solve_ref.precond_inverse(B, nv, 2)[0] @ B
        y = np.random.default_rng(8).standard_normal(B.shape[0])
        assert np.abs(g.apply(Bh @ y) - y).max() <= 1e-12 * np.abs(y).max()


def test_the_indefinite_case_still_does_not_converge(oracle):
    """ripf_tet_dt01 (Courant 900, negative diagonal entries): ILU(0) does not rescue it -- DESIGN.md 7.1, Limits found"""
    s = solve_systems.get("ripf_tet_dt01")
    rp, col, val, rhs = s.oracle_assemble(oracle)
    A = sps.csr_matrix((val, col, rp), shape=(rhs.size, rhs.size))
    x, info = solve_ref_ilu.bicgstab(A, rhs, np.zeros(rhs.size), 1e-8, nv=s.nv, max_its=300)
    print("ripf_tet_dt01:", info)
    assert info["reason"] == solve_ref_ilu.MAX_ITS and info["iterations"] == 300
    assert info["residual_norm"] > 1e-4 * info["rhs_norm"]
