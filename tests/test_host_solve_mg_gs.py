"""CPU build of the colouring of the Gauss-Seidel smoother (rdcfes_amd/csrc/rdc_solve.h: mg_colour, mg_gs_place;
tests/host_solve_mg_gs_shim.cpp) as compiled by g++: the colours and colour lists of every level held exactly against the numpy
restatement (tests/solve_ref_mg_gs.py: colour) on the block patterns of K(8), the hydrogel mesh and the hub mesh; the refusal of
a structurally asymmetric pattern; and the placement of the lists in their one allocation."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import meshes
import solve_ref_mg
import solve_ref_mg_gs
from rdcfes_amd import synth

ROOT = Path(__file__).resolve().parent.parent
LISTS = {"colour": (0, np.int32), "cptr": (1, np.int64), "nodes": (2, np.int32)}


@pytest.fixture(scope="module")
def lib():
    out = ROOT / "tests" / "_build" / "libhost_solve_mg_gs_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_solve_mg_gs_shim.cpp"
    hdr = ROOT / "rdcfes_amd" / "csrc" / "rdc_solve.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        str(src), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.shim_gs_colour.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
    lib.shim_gs_colour_one.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
    lib.shim_gs_list.restype = C.c_int64
    lib.shim_gs_list.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.shim_gs_place.restype = C.c_int64
    lib.shim_gs_place.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    return lib


def _patterns():
    conn, xyz = synth.kuhn_tet_mesh(8, order="random")
    yield "pihna_kuhn8", 4, conn, xyz.shape[0], 5
    conn, xyz = meshes.hydrogel()
    yield "pihna_hydrogel", 4, conn, xyz.shape[0], 5
    conn, xyz = meshes.hub(max(meshes.HUB_TETS.values()))
    yield "pihna_hub", 4, conn, xyz.shape[0], 5


def _colour(lib, bptr, bcol):
    """[dict(colour, cptr, nodes)] per level from the compiled code"""
    n_levels = lib.shim_gs_colour(bptr.size - 1, bptr.ctypes.data, bcol.ctypes.data)
    assert n_levels >= 1
    out = []
    for l in range(n_levels):
        lv = {}
        for name, (which, dt) in LISTS.items():
            a = np.empty(lib.shim_gs_list(l, which, None), dtype=dt)
            assert lib.shim_gs_list(l, which, a.ctypes.data) == a.size
            lv[name] = a
        out.append(lv)
    return out


def test_constants(lib):
    c = (C.c_int * 2)()
    assert lib.shim_gs_constants(c) == 2 and list(c) == [512, 256]


@pytest.mark.parametrize("case", list(_patterns()), ids=lambda c: c[0])
def test_colours_against_numpy_and_their_placement(oracle, lib, case):
    name, et, conn, nn, nv = case
    _, _, bptr, bcol = oracle.build_pattern(et, conn, nn, nn, nv)
    bptr, bcol = np.ascontiguousarray(bptr, dtype=np.int64), np.ascontiguousarray(bcol, dtype=np.int32)
    got = _colour(lib, bptr, bcol)
    levels = [(bptr, bcol)] + [(st["bptr"], st["bcol"]) for st in solve_ref_mg.pattern_hierarchy(bptr, bcol)]
    print(name, "colours per level:", [lv["cptr"].size - 1 for lv in got])
    assert len(got) == len(levels) >= 3
    for lv, (fb, fc) in zip(got, levels):
        col, cptr, nodes = solve_ref_mg_gs.colour(fb, fc)
        np.testing.assert_array_equal(lv["colour"], col, err_msg=name)
        np.testing.assert_array_equal(lv["cptr"], cptr, err_msg=name)
        np.testing.assert_array_equal(lv["nodes"], nodes, err_msg=name)
        assert solve_ref_mg_gs.is_proper(fb, fc, lv["colour"]) and cptr.size - 1 <= np.diff(fb).max()
    if name == "pihna_hub":
        assert np.diff(bptr).max() >= 740
    # placement: measured first, then placed into an arena of exactly the measured size, offsets aligned, in bounds, disjoint
    nbytes = lib.shim_gs_place(None, 0, None, None)
    assert nbytes > 0 and nbytes % 256 == 0
    assert nbytes >= sum(4 * lv["nodes"].size + 8 * lv["cptr"].size for lv in got)
    assert nbytes <= sum(4 * lv["nodes"].size + 8 * lv["cptr"].size + 2 * 255 for lv in got)
    arena = np.full(nbytes, 0x5A, dtype=np.uint8)
    off, ncol = np.zeros(2 * len(got), dtype=np.int64), np.zeros(len(got), dtype=np.int32)
    assert lib.shim_gs_place(arena.ctypes.data, nbytes - 1, off.ctypes.data, ncol.ctypes.data) == -1
    assert lib.shim_gs_place(arena.ctypes.data, nbytes, off.ctypes.data, ncol.ctypes.data) == nbytes
    spans = []
    for l, lv in enumerate(got):
        assert ncol[l] == lv["cptr"].size - 1
        for at, a in ((off[2 * l], lv["nodes"]), (off[2 * l + 1], lv["cptr"])):
            assert at % 256 == 0 and 0 <= at and at + a.nbytes <= nbytes
            assert arena[at:at + a.nbytes].tobytes() == a.tobytes()
            spans.append((int(at), int(at) + a.nbytes))
    spans.sort()
    assert all(e0 <= s1 for (_, e0), (s1, _) in zip(spans, spans[1:]))


def test_asymmetric_pattern_is_refused(oracle, lib):
    """one block removed on one side: greedy colours in ascending order, so the later node of such a pair does not see the earlier
    one.  Of the pairs (i, j), i < j, whose two nodes then take the same colour, the first is the witness"""
    name, et, conn, nn, nv = next(_patterns())
    _, _, bptr, bcol = oracle.build_pattern(et, conn, nn, nn, nv)
    bptr, bcol = np.ascontiguousarray(bptr, dtype=np.int64), np.ascontiguousarray(bcol, dtype=np.int32)
    assert lib.shim_gs_colour_one(nn, bptr.ctypes.data, bcol.ctypes.data) == 1
    refused = 0
    for j in range(nn - 1, nn - 40, -1):           # remove block (j, i), i the first neighbour below j; (i, j) stays
        row = bcol[bptr[j]:bptr[j + 1]]
        k = int(bptr[j]) + int(np.flatnonzero(row < j)[0])
        cut_col = np.delete(bcol, k)
        cut_ptr = bptr.copy()
        cut_ptr[j + 1:] -= 1
        col, _, _ = solve_ref_mg_gs.colour(cut_ptr, cut_col)
        proper = solve_ref_mg_gs.is_proper(cut_ptr, cut_col, col)
        assert lib.shim_gs_colour_one(nn, cut_ptr.ctypes.data, cut_col.ctypes.data) == int(proper)
        refused += not proper
    assert refused >= 1
