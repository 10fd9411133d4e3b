"""The numpy yardstick of the multigrid solve across ranks (tests/solve_ref_mg_dist.py) against the global emulation of the same
method (rank-local aggregates in ONE solve_ref_mg.Hierarchy, nodes ordered rank by rank) and against the block-Jacobi yardstick
of solve_ref_dist, on the partitions the GPU tests use."""
import numpy as np
import pytest

import solve_ref
import solve_ref_dist
import solve_ref_mg
import solve_ref_mg_dist
from solve_ref_dist import global_system, ranks_of

ROWS = [("pihna_kuhn", 1), ("pihna_kuhn", 2), ("pihna_kuhn", 3), ("hcc_hex", 2), ("hcc_hex", 3), ("pihna_kuhn3", 3)]
_H = {}


def hierarchy(name, world, oracle):
    if (name, world) not in _H:
        s = solve_ref_dist.case(name)
        _H[(name, world)] = solve_ref_mg_dist.HierarchyDist(ranks_of(name, world, oracle), s.nv)
    return _H[(name, world)]


@pytest.mark.parametrize("name,world", ROWS)
def test_yardstick_equals_the_global_emulation(oracle, name, world):
    s, A, b = global_system(name, oracle)
    ranks = ranks_of(name, world, oracle)
    H = hierarchy(name, world, oracle)
    n_node = s.xyz.shape[0]
    for rel_tol in (1e-8, 1e-10):
        H.exchanges = [0] * H.n_levels
        xs, info = solve_ref_mg_dist.bicgstab_dist(ranks, [np.zeros(rk.A.shape[1]) for rk in ranks], rel_tol, nv=s.nv, hierarchy=H)
        x = solve_ref_dist.gather(ranks, xs, s.nv, n_node)
        xe, emu, E = solve_ref_mg_dist.emulate(A, b, ranks, s.nv, rel_tol)
        _, jac = solve_ref_dist.yardstick(name, oracle, rel_tol)
        f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
        sizes = [sum(H.level_sizes(r)[l][0] for r in range(world)) for l in range(H.n_levels)]
        print(f"{s.name} world {world} tol {rel_tol:g}: multigrid {info['iterations']} (restarts {info['restarts']}), emulation "
              f"{emu['iterations']}, block Jacobi {jac['iterations']}; levels {sizes}; complexity {emu['complexity']:.3f}; "
              f"|x - x_emulation| / |x| {np.linalg.norm(x - xe) / np.linalg.norm(xe):.2e}; residual {f['residual_norm']:.3e} <= {f['bound']:.3e}")
        assert info["reason"] == solve_ref.CONVERGED and emu["reason"] == solve_ref.CONVERGED
        assert info["iterations"] == emu["iterations"] and info["restarts"] == emu["restarts"]
        # the same arithmetic up to the order of sums: the two x differ by rounding amplified by the iteration, far below the tolerance
        assert np.linalg.norm(x - xe) <= 1e-3 * rel_tol * np.linalg.norm(xe)
        assert info["iterations"] <= jac["iterations"]
        assert sizes == [n for n, _ in E.level_sizes()]
        assert [sum(H.level_sizes(r)[l][1] for r in range(world)) for l in range(H.n_levels)] == [nb for _, nb in E.level_sizes()]
        for l in range(H.n_levels):
            assert [H.level_sizes(r)[l][0] for r in range(world)] == E.counts[l]
        # exchanges: per iteration 6 on level 0 (2 per cycle, 2 outer) and 2 (2 (L - 2) + 7) below; one more on level 0 per true residual
        L, its = H.n_levels, info["iterations"]
        assert L >= 2 and sum(H.exchanges[1:]) == 2 * (2 * (L - 2) + 7) * its
        assert H.exchanges[0] == 6 * its


def test_world_1_is_the_single_partition_hierarchy(oracle):
    for name in ("pihna_kuhn", "hcc_hex"):
        s = solve_ref_dist.case(name)
        H = hierarchy(name, 1, oracle)
        rk = ranks_of(name, 1, oracle)[0]
        bptr, bcol, _ = solve_ref_mg.block_pattern(rk.A, s.nv)
        ref = solve_ref_mg.pattern_hierarchy(bptr, bcol)
        assert len(H.steps[0]) == len(ref) >= 2
        for st, rf in zip(H.steps[0], ref):
            assert st["n"] == rf["n"] and st["n_pass1"] == rf["n_pass1"]
            for key in ("agg", "bptr", "bcol", "cptr", "cidx"):
                np.testing.assert_array_equal(st[key], rf[key], err_msg=f"{name} {key}")
        assert all(h["n_ghost"] == 0 and h["send_nodes"].size == 0 and not h["peers"] for h in H.halos[0])


@pytest.mark.parametrize("name,world", [r for r in ROWS if r[1] > 1])
def test_ghost_layers_pair_up_on_every_level(oracle, name, world):
    """rank r's send segment for q and q's ghost segment from r name the same aggregates in the same order; the tail is grouped by
    owner; every ghost column of a coarse row is one of the coarse ghosts"""
    H = hierarchy(name, world, oracle)
    for l in range(H.n_levels):
        for r in range(world):
            hr = H.halos[r][l]
            assert hr["ghost_off"][-1] == hr["n_ghost"] and hr["send_off"][-1] == hr["send_nodes"].size
            np.testing.assert_array_equal(hr["send_nodes"][hr["send_slot"]], np.repeat(np.arange(hr["n"]), np.diff(hr["send_ptr"])))
            for k, q in enumerate(hr["peers"]):
                hq = H.halos[q][l]
                j = hq["peers"].index(r)
                assert hr["send_off"][k + 1] - hr["send_off"][k] == hq["ghost_off"][j + 1] - hq["ghost_off"][j]
                if l:      # the coarse ghosts of q from r ARE r's send list for q: distinct aggregates of r, first appearance
                    sent, got = H.ids[r][l - 1][0], H.ids[q][l - 1][1]
                    fr, fq = H.halos[r][l - 1], H.halos[q][l - 1]
                    a = solve_ref_mg_dist.first_appearance(sent[fr["send_off"][k]:fr["send_off"][k + 1]].astype(np.int64))[0]
                    g = solve_ref_mg_dist.first_appearance(got[fq["ghost_off"][j]:fq["ghost_off"][j + 1]].astype(np.int64))[0]
                    np.testing.assert_array_equal(a, g)
                    np.testing.assert_array_equal(hr["send_nodes"][hr["send_off"][k]:hr["send_off"][k + 1]], a)
            if l:
                st = H.steps[r][l - 1]
                assert st["bcol"].size == 0 or st["bcol"].max() < hr["n"] + hr["n_ghost"]
