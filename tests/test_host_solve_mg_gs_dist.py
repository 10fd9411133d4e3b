"""CPU build of what the rank-local Gauss-Seidel smoother across ranks (precond 6) adds on the host
(tests/host_solve_mg_gs_dist_shim.cpp: mg_colour on the levels of every rank's partitioned hierarchy, mg_gs_interior, mg_gs_place)
against the numpy yardstick tests/solve_ref_mg_gs_dist.py, and the validity rule of rdc_solve_state.h for the new value (through
tests/host_solve_state_shim.cpp, next to tests/test_host_solve_state.py): a call with precond 6 leaves what its precond-3 row leaves."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import solve_ref_dist
import solve_ref_mg
import solve_ref_mg_gs_dist as Y
from test_host_solve_mg_dist import _build, _unconnected_world

ROOT = Path(__file__).resolve().parent.parent
LISTS = {"colour": (0, np.int32), "cptr": (1, np.int64), "nodes": (2, np.int32)}


def _compile(name, deps, flags=()):
    out = ROOT / "tests" / "_build" / f"lib{name}.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / f"{name}.cpp"
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in [src] + deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", *flags, str(src), "-o", str(out)], check=True)
    return C.CDLL(str(out))


@pytest.fixture(scope="module")
def lib():
    lib = _compile("host_solve_mg_gs_dist_shim", [ROOT / "tests" / "host_solve_mg_dist_shim.cpp", ROOT / "rdcfes_amd" / "csrc" / "rdc_solve.h"],
                   ("-ffp-contract=off", "-Wno-unknown-pragmas"))
    lib.shim_dist_plan.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.shim_dist_aggregate.restype = C.c_int64
    lib.shim_dist_aggregate.argtypes = [C.c_int, C.c_void_p]
    lib.shim_dist_coarsen.argtypes = [C.c_int, C.c_void_p]
    lib.shim_dist_goes_on.argtypes = [C.c_int, C.c_double, C.c_double]
    lib.shim_dist_list.restype = C.c_int64
    lib.shim_dist_list.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.shim_gsd_list.restype = C.c_int64
    lib.shim_gsd_list.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.shim_gsd_interior.restype = C.c_int64
    lib.shim_gsd_interior.argtypes = [C.c_int, C.c_int64]
    lib.shim_gsd_place.restype = C.c_int64
    lib.shim_gsd_place.argtypes = [C.c_int, C.c_void_p]
    return lib


def _gs_list(lib, r, level, key):
    which, dt = LISTS[key]
    a = np.empty(lib.shim_gsd_list(r, level, which, None), dtype=dt)
    assert lib.shim_gsd_list(r, level, which, a.ctypes.data) == a.size
    return a


def _align(nbytes):
    return (nbytes + 255) // 256 * 256


@pytest.mark.parametrize("name,world", [("pihna_kuhn", 2), ("pihna_kuhn", 3), ("hcc_hex", 2), ("hcc_hex", 3), ("pihna_kuhn3", 3)])
def test_colours_of_every_rank_and_level_against_numpy(oracle, lib, name, world):
    s = solve_ref_dist.case(name)
    ranks = solve_ref_dist.ranks_of(name, world, oracle)
    _, H = Y.hierarchy(name, world, oracle)
    patterns = [solve_ref_mg.block_pattern(rk.A, s.nv)[:2] for rk in ranks]
    levels = _build(lib, patterns, [rk.lp for rk in ranks])
    assert levels == H.n_levels
    for r, rk in enumerate(ranks):
        assert lib.shim_gsd_colour(r) == levels
        for l in range(levels):
            for key, want in zip(("colour", "cptr", "nodes"), H.cols[r][l]):
                np.testing.assert_array_equal(_gs_list(lib, r, l, key), want, err_msg=f"rank {r} level {l} {key}")
        # the part of colour 0 that runs inside the exchange of level 0
        col, cptr, nodes = H.cols[r][0]
        first = nodes[cptr[0]:cptr[1]]
        for n_int in (0, rk.lp.n_interior, rk.lp.n_owned, rk.lp.n_owned + 5):
            assert lib.shim_gsd_interior(r, n_int) == int(np.searchsorted(first, n_int)) == Y.interior_split(nodes, cptr, n_int)
        # an arena of exactly the measured size: every list 256-aligned, nothing else
        n_colours = (C.c_int32 * levels)()
        want_bytes = sum(_align(4 * c[2].size) + _align(8 * c[1].size) for c in H.cols[r])
        assert lib.shim_gsd_place(r, n_colours) == want_bytes
        assert list(n_colours) == H.colours(r)
    print(name, world, "colours per rank:", [H.colours(r) for r in range(world)],
          "interior of colour 0:", [lib.shim_gsd_interior(r, rk.lp.n_interior) for r, rk in enumerate(ranks)])
    if name == "pihna_kuhn3":      # a rank without an interior: nothing of its sweep runs inside the exchange
        assert any(rk.lp.n_interior == 0 and lib.shim_gsd_interior(r, rk.lp.n_interior) == 0 for r, rk in enumerate(ranks))


def test_a_rank_of_unconnected_nodes_has_one_colour(lib):
    patterns, lps = _unconnected_world()
    levels = _build(lib, patterns, lps)
    assert lib.shim_gsd_colour(0) == levels and lib.shim_gsd_colour(1) == levels
    # rank 1's nodes are coupled to ghosts only: the owned square is diagonal
    np.testing.assert_array_equal(_gs_list(lib, 1, 0, "colour"), np.zeros(10, dtype=np.int32))
    np.testing.assert_array_equal(_gs_list(lib, 1, 0, "cptr"), [0, 10])
    assert _gs_list(lib, 0, 0, "cptr").size - 1 == 2      # a 5-point grid graph is bipartite
    n_colours = (C.c_int32 * levels)()
    assert lib.shim_gsd_place(1, n_colours) > 0 and n_colours[0] == 1


def test_an_owned_square_that_is_not_symmetric_is_refused(lib):
    """rank 0 owns 3 nodes; node 0 names node 2 but not the reverse: greedy gives both colour 0.  The asymmetry in a GHOST column
    (node 1 names ghost 3) is not looked at."""
    rows = [[0, 2], [1, 3], [2]]
    bptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    bcol = np.concatenate(rows).astype(np.int32)
    send, one = np.array([1], dtype=np.int32), np.array([1], dtype=np.int64)
    lib.shim_dist_world(1)
    assert lib.shim_dist_plan(0, 3, 1, bptr.ctypes.data, bcol.ctypes.data, 1, send.ctypes.data, 1, one.ctypes.data, one.ctypes.data) == 0
    assert lib.shim_gsd_colour(0) == -2
    rows[2] = [0, 2]
    bptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    bcol = np.concatenate(rows).astype(np.int32)
    assert lib.shim_dist_plan(0, 3, 1, bptr.ctypes.data, bcol.ctypes.data, 1, send.ctypes.data, 1, one.ctypes.data, one.ctypes.data) == 0
    assert lib.shim_gsd_colour(0) == 1
    np.testing.assert_array_equal(_gs_list(lib, 0, 0, "colour"), [0, 0, 1])


# ---- the validity rule: precond 6 next to precond 3 ----
SCALE_F32, SOLVE, ARNOLDI, MG_APPLY, ILU_APPLY, DIST, DIST_PLAN = range(7)
CONVERGED, BAD_DIAGONAL = 0, 3


@pytest.fixture(scope="module")
def state():
    csrc = ROOT / "rdcfes_amd" / "csrc"
    lib = _compile("host_solve_state_shim", [csrc / "rdc_options.h", csrc / "rdc_solve_state.h", ROOT / "include" / "rdc_assembly.h"])
    lib.shim_valid_apply.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.shim_valid_apply.restype = None
    return lib


def _apply(state, flags, entry, precond, mixed, gmres, stage, outcome):
    f, o = (C.c_int * 6)(*flags), (C.c_int * 7)(*outcome)
    state.shim_valid_apply(f, entry, precond, int(mixed), int(gmres), stage, o)
    return tuple(f)


@pytest.mark.parametrize("label,entry", [("solve", SOLVE), ("dist", DIST), ("arnoldi", ARNOLDI)])
def test_precond_6_leaves_what_precond_3_leaves(state, label, entry):
    all_valid, nothing = (1, 1, 1, 1, 30, 2), (0, 0, 0, 0, 0, 0)
    outcomes = [(1, 0, 0, 64, CONVERGED, 30, 1), (1, 0, 0, 32, CONVERGED, 12, 3), (1, 0, 0, 64, BAD_DIAGONAL, 30, 1), (1, 0, 2, 32, CONVERGED, 30, 1),
                (0, 0, 0, 64, CONVERGED, 30, 1), (1, 1, 0, 64, CONVERGED, 30, 1)]
    for flags, mixed, gmres, stage, outcome in itertools.product((all_valid, nothing), (False, True), (False, True), (0, 1, 2), outcomes):
        gmres = gmres or entry == ARNOLDI
        assert _apply(state, flags, entry, 6, mixed, gmres, stage, outcome) == _apply(state, flags, entry, 3, mixed, gmres, stage, outcome)
    # literals: a solve with 6 on one partition leaves levels that can be downloaded, a partitioned one does not; neither touches
    # the ILU(0) factor; a mixed one that ran leaves a usable fp32 copy
    ran = (1, 0, 0, 32, CONVERGED, 30, 1)
    assert _apply(state, nothing, SOLVE, 6, True, False, 2, ran)[:3] == (1, 1, 0)
    assert _apply(state, all_valid, DIST, 6, True, False, 2, ran)[:3] == (1, 0, 1)
    assert _apply(state, all_valid, ARNOLDI, 6, False, True, 2, (1, 0, 0, 64, CONVERGED, 0, 0))[:3] == (1, 1, 1)
    assert _apply(state, all_valid, SOLVE, 6, False, False, 0, ran)[:3] == (1, 0, 1)      # refused behind the entry: the levels are gone
    # the value is a multigrid value and no ILU value: precond 5 differs where the factor is concerned
    assert _apply(state, all_valid, DIST, 5, False, False, 1, ran)[2] == 0 and _apply(state, all_valid, DIST, 6, False, False, 1, ran)[2] == 1
