"""tests/solve_ref_gmres_dist.py -- the numpy yardstick of tests/test_gpu_solve_dist_gmres.py -- pinned on the CPU on oracle-assembled
systems: every case the GPU test runs converges in the yardstick, with the Arnoldi steps and restarts on record here (the GPU test
is held to steps <= these + 2, and to these restarts whenever the steps are equal); the residual inequality of the solver tests; the
right preconditioners on global vectors against the per-rank forms they wrap; and, with one rank, the single-partition yardstick."""
import numpy as np
import pytest

import solve_ref
import solve_ref_dist
import solve_ref_gmres
import solve_ref_gmres_dist as G
import solve_ref_ilu
import solve_ref_mg_dist

# (iterations, restarts) at rel_tol 1e-8 and 1e-10, in the order of G.CASES
RECORD = {
    ("pihna_kuhn", 2, 2, 30, False): ((41, 1), (51, 1)), ("pihna_kuhn", 2, 5, 30, False): ((16, 0), (20, 0)),
    ("pihna_kuhn", 2, 3, 30, False): ((15, 0), (19, 0)), ("pihna_kuhn", 3, 2, 30, False): ((41, 1), (51, 1)),
    ("pihna_kuhn", 3, 5, 30, False): ((17, 0), (21, 0)), ("pihna_kuhn", 3, 3, 30, False): ((15, 0), (19, 0)),
    ("hcc_hex", 2, 2, 30, False): ((40, 1), (52, 1)), ("hcc_hex", 2, 5, 30, False): ((12, 0), (15, 0)),
    ("hcc_hex", 2, 3, 30, False): ((20, 0), (25, 0)), ("pihna_kuhn3", 3, 2, 30, False): ((14, 0), (17, 0)),
    ("pihna_kuhn3", 3, 5, 30, False): ((9, 0), (12, 0)), ("pihna_kuhn3", 3, 3, 30, False): ((9, 0), (11, 0)),
    ("pihna_kuhn", 2, 2, 7, True): ((49, 6), (62, 8)),
}


def test_the_record_covers_the_cases():
    assert set(RECORD) == set(G.CASES) and len(G.CASES) == 13
    counts = [c for row in RECORD.values() for c in row]
    assert any(r == 0 for _, r in counts) and any(r >= 1 for _, r in counts)     # restart-free and restarted examples
    assert not any(name == "pihna_hydrogel" for name, *_ in G.CASES)


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_cases_converge_with_the_recorded_counts(oracle, case):
    name, world, precond, restart, refine = case
    s, A, b = solve_ref_dist.global_system(name, oracle)
    for rel_tol, want in zip(G.TOLS, RECORD[case]):
        x, info = G.gmres_dist(name, world, oracle, rel_tol, precond, restart, refine)
        print(f"{name} world {world} precond {precond} restart {restart} refine {refine} tol {rel_tol:g}: {info['iterations']} steps, "
              f"{info['restarts']} restarts")
        assert info["reason"] == solve_ref_gmres.CONVERGED, info
        assert (info["iterations"], info["restarts"]) == want, (info, want)
        assert info["restarts"] == (info["iterations"] - 1) // restart
        f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
        assert abs(info["residual_norm"] - f["residual_norm"]) <= f["rho"]


def test_right_preconditioners_on_global_vectors(oracle):
    """the wrappers move nothing but rows: precond 5 is every rank's factor on its own rows, precond 3 the cycle of the ranks"""
    name, world = "pihna_kuhn", 3
    s = solve_ref_dist.case(name)
    ranks = solve_ref_dist.ranks_of(name, world, oracle)
    dofs = G.rank_dofs(ranks, s.nv)
    assert np.array_equal(np.sort(np.concatenate(dofs)), np.arange(s.xyz.shape[0] * s.nv))     # every global dof is owned once
    y = np.random.default_rng(4).standard_normal(s.xyz.shape[0] * s.nv)
    z5, z3 = G.right_of(ranks, s.nv, 5)(y), G.right_of(ranks, s.nv, 3)(y)
    parts3 = solve_ref_mg_dist.HierarchyDist(ranks, s.nv).cycle([y[d] for d in dofs])
    for r, (rk, d) in enumerate(zip(ranks, dofs)):
        f = solve_ref_ilu.Factor(rk.A[:, :rk.lp.n_owned * s.nv].tocsr(), s.nv)
        assert z5[d].tobytes() == f.apply(y[d]).tobytes(), r
        assert z3[d].tobytes() == parts3[r].tobytes(), r
    assert G.right_of(ranks, s.nv, 2) is None


def test_one_rank_is_the_single_partition_yardstick(oracle):
    name = "pihna_kuhn"
    s, A, b = solve_ref_dist.global_system(name, oracle)
    for precond, right in ((2, None), (5, solve_ref_ilu.Factor(A, s.nv).apply)):
        x1, i1 = G.gmres_dist(name, 1, oracle, 1e-8, precond)
        x0, i0 = solve_ref_gmres.gmres(A, b, np.zeros(b.size), 1e-8, max_its=2000, precond=2, nv=s.nv, right=right)
        assert (i1["iterations"], i1["restarts"]) == (i0["iterations"], i0["restarts"])
        assert np.linalg.norm(x1 - x0) <= 1e-10 * np.linalg.norm(x0)


def test_arnoldi_operators_in_rank_order(oracle):
    """operators(): FP64 and extended precision agree to rounding, for every preconditioner the hook is tested with"""
    name, world = "pihna_kuhn", 2
    s, A, b = solve_ref_dist.global_system(name, oracle)
    ranks = solve_ref_dist.ranks_of(name, world, oracle)
    perm, counts = solve_ref_mg_dist.rank_order(ranks)
    dof = (perm[:, None] * s.nv + np.arange(s.nv)).reshape(-1)
    Ap = A[dof][:, dof].tocsr()
    v = np.random.default_rng(8).standard_normal(b.size)
    for precond in (2, 5, 3):
        op, op_ld = G.operators(Ap, counts, s.nv, precond)
        w, wl = op(v), op_ld(v)
        assert wl.dtype == np.longdouble
        d = np.asarray(w, dtype=np.longdouble) - wl
        assert float(np.sqrt(d @ d) / np.sqrt(wl @ wl)) <= 1e-12, precond
    # in rank order the right preconditioner of 5 is that of the yardstick on global vectors
    op5 = G.operators(Ap, counts, s.nv, 5)[0]
    M = solve_ref.precond_inverse(A, s.nv, 2)[0]
    want = (M @ (A @ G.right_of(ranks, s.nv, 5)(b)))[dof]
    got = op5(b[dof])
    assert np.linalg.norm(got - want) <= 1e-9 * np.linalg.norm(want)
