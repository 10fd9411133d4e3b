"""The numpy yardstick of the rank-local Gauss-Seidel smoother across ranks (tests/solve_ref_mg_gs_dist.py; precond 6) on the
partitions the GPU tests use: its table of iteration counts, its colours, its exchange counts, world 1 against the single-partition
yardstick tests/solve_ref_mg_gs.py, and its two restatements (per rank with exchanges; one global hierarchy in rank order, FP64
and extended precision) against each other."""
import numpy as np
import pytest

import solve_ref
import solve_ref_dist
import solve_ref_mg_dist
import solve_ref_mg_gs
import solve_ref_mg_gs_dist as Y
import solve_ref_mg_ld as ld
from solve_ref_dist import global_system, ranks_of

ROWS = sorted(Y.TABLE)


@pytest.mark.parametrize("name,world", ROWS)
def test_table_of_the_yardstick(oracle, name, world):
    s, A, b = global_system(name, oracle)
    ranks = ranks_of(name, world, oracle)
    base, H = Y.hierarchy(name, world, oracle)
    row = Y.TABLE[(name, world)]
    n_node = s.xyz.shape[0]
    got = dict(jacobi=[], bicgstab=[], gmres=[])
    for rel_tol in Y.TOLS:
        xs, info = Y.bicgstab(name, world, oracle, rel_tol)
        exchanges = list(info["level_exchanges"])
        _, jac = Y.bicgstab(name, world, oracle, rel_tol, smoother=0)
        x = solve_ref_dist.gather(ranks, xs, s.nv, n_node)
        f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
        print(f"{name} world {world} tol {rel_tol:g}: BiCGStab {info['iterations']} (restarts {info['restarts']}), Jacobi smoother {jac['iterations']}; "
              f"levels {H.n_levels}; colours {[H.colours(r) for r in range(world)]}; exchanges per level {exchanges}; residual "
              f"{f['residual_norm']:.3e} <= {f['bound']:.3e}")
        assert info["reason"] == solve_ref.CONVERGED and info["restarts"] == 0
        assert jac["reason"] == solve_ref.CONVERGED and info["iterations"] <= jac["iterations"]
        # exchanges: those of the Jacobi cycle (tests/test_solve_ref_mg_dist.py), count for count: the smoother costs no message
        L, its = H.n_levels, info["iterations"]
        assert L >= 2 and sum(exchanges[1:]) == 2 * (2 * (L - 2) + 7) * its and exchanges[0] == 6 * its
        assert jac["level_exchanges"][0] == 6 * jac["iterations"] and sum(jac["level_exchanges"][1:]) == 2 * (2 * (L - 2) + 7) * jac["iterations"]
        got["jacobi"].append(jac["iterations"])
        got["bicgstab"].append(info["iterations"])
        if row["gmres"] is not None:
            xg, gi = Y.gmres(name, world, oracle, rel_tol)
            _, gj = Y.gmres(name, world, oracle, rel_tol, smoother=0)
            fg = solve_ref.check_solution(A, b, xg, s.nv, 2, rel_tol)
            print(f"    GMRES(30) {gi['iterations']} (restarts {gi['restarts']}), Jacobi smoother {gj['iterations']}; residual {fg['residual_norm']:.3e} "
                  f"<= {fg['bound']:.3e}")
            assert gi["reason"] == solve_ref.CONVERGED and gi["restarts"] == 0
            assert gj["reason"] == solve_ref.CONVERGED and gi["iterations"] <= gj["iterations"]
            got["gmres"].append(gi["iterations"])
    assert tuple(got["jacobi"]) == row["jacobi"] and tuple(got["bicgstab"]) == row["bicgstab"], got
    assert row["gmres"] is None or tuple(got["gmres"]) == row["gmres"], got
    assert H.n_levels == row["levels"] and [H.colours(r) for r in range(world)] == row["colours"]


@pytest.mark.parametrize("name,world", ROWS)
def test_colourings_are_proper_and_per_rank(oracle, name, world):
    _, H = Y.hierarchy(name, world, oracle)
    for r, rk in enumerate(ranks_of(name, world, oracle)):
        for l in range(H.n_levels):
            bptr, bcol = H.pattern(r, l)
            col, cptr, nodes = H.cols[r][l]
            n = H.lv[r][l]["n"]
            assert col.size == n == bptr.size - 1 and cptr[-1] == n
            assert solve_ref_mg_gs.is_proper(np.asarray(bptr), np.asarray(bcol), col), f"rank {r} level {l}"
            assert np.array_equal(np.sort(nodes), np.arange(n))
            for c in range(cptr.size - 1):
                part = nodes[cptr[c]:cptr[c + 1]]
                assert part.size and np.all(col[part] == c) and np.all(np.diff(part) > 0)
        # the nodes of colour 0 of level 0 that read no ghost are a prefix of its list
        col, cptr, nodes = H.cols[r][0]
        k = Y.interior_split(nodes, cptr, rk.lp.n_interior)
        first = nodes[cptr[0]:cptr[1]] if cptr.size > 1 else nodes[:0]
        assert np.all(first[:k] < rk.lp.n_interior) and np.all(first[k:] >= rk.lp.n_interior)
        assert solve_ref_dist.interior_rows_read_no_ghost(rk, H.nv)


def test_world_1_is_the_single_partition_smoother(oracle):
    name = "pihna_kuhn"
    s, A, b = global_system(name, oracle)
    rk = ranks_of(name, 1, oracle)[0]
    _, H = Y.hierarchy(name, 1, oracle)
    ref = solve_ref_mg_gs.Hierarchy(rk.A, s.nv)
    assert H.colours(0) == ref.colours()
    for l, lv in enumerate(ref.levels):
        for got, want in zip(H.cols[0][l], (lv["colour"], lv["cptr"], lv["cnodes"])):
            np.testing.assert_array_equal(got, want)
    for rel_tol in Y.TOLS:
        xs, info = Y.bicgstab(name, 1, oracle, rel_tol)
        x1, one = solve_ref_mg_gs.bicgstab(rk.A, rk.b, np.zeros(rk.b.size), rel_tol, nv=s.nv, hierarchy=ref)
        d = np.linalg.norm(xs[0] - x1) / np.linalg.norm(x1)
        print(f"world 1 tol {rel_tol:g}: {info['iterations']} iterations, single partition {one['iterations']}; |x - x_single| / |x| {d:.2e}")
        assert info["iterations"] == one["iterations"] and info["restarts"] == one["restarts"] and one["reason"] == solve_ref.CONVERGED
        assert d <= 1e-3 * rel_tol      # the same arithmetic up to the order of sums, amplified by the iteration


@pytest.mark.parametrize("name,world", [("pihna_kuhn", 2), ("pihna_kuhn", 3), ("hcc_hex", 2), ("hcc_hex", 3)])
def test_global_emulation_and_extended_precision(oracle, name, world):
    """the cycle per rank with exchanges = the cycle of one global hierarchy in rank order, to rounding; and the extended-precision
    evaluation of the latter stands where numpy's FP64 stands, up to FP64 rounding.  Bounds: the two FP64 evaluations do the same
    arithmetic up to the order of the sums of a row (at most 27 x 5 terms) through 3 levels and 9 sweeps, a few thousand roundings
    in a row: 1e-12 = 4500 eps; the distance from extended precision also carries the conditioning of every D_l^-1, which
    solve_ref_mg_ld.BOUND_CAP lets be 1e-6 / 128: 1e-10 is below that.  (K(3) is left out: its 64-node system amplifies the rounding of
    a random input to 1e-5 under the damped-Jacobi smoother just as under this one, so it shows nothing about the sweep.)"""
    s, A, b = global_system(name, oracle)
    ranks = ranks_of(name, world, oracle)
    _, H = Y.hierarchy(name, world, oracle)
    perm, counts = solve_ref_mg_dist.rank_order(ranks)
    dof = (perm[:, None] * s.nv + np.arange(s.nv)).reshape(-1)
    Ap = A[dof][:, dof].tocsr()
    E = Y.EmulatedGs(Ap, s.nv, counts)
    C = Y.CycleLocal(E, Ap)
    off = np.concatenate([[0], np.cumsum(counts)]) * s.nv
    for l in range(H.n_levels):
        for r in range(world):
            assert len(E.levels[l]["rank_nodes"][r]) == H.colours(r)[l]
    for v in ld.probe_vectors(b.size, b[dof]):
        z_ranks = np.concatenate(H.cycle([v[off[r]:off[r + 1]] for r in range(world)]))
        z, z_ld = E.cycle(v), C.cycle(v)
        d, noise = ld.rel_diff(z_ranks, z.astype(ld.LD)), ld.rel_diff(z, z_ld)
        print(f"{name} world {world}: per rank against global {max(d):.2e}, FP64 against extended precision {max(noise):.2e}")
        assert max(d) <= 1e-12 and max(noise) <= 1e-10
