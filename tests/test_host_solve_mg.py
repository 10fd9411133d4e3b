"""CPU build of the multigrid part of rdcfes_amd/csrc/rdc_solve.h (tests/host_solve_mg_shim.cpp): the aggregation, the coarse
patterns and the contribution lists of the Galerkin kernel as compiled by g++, held exactly against the numpy restatement
(tests/solve_ref_mg.py) on the block patterns of K(8), the jittered HEX8 mesh, the hub mesh and the hydrogel mesh; the
properties of a valid hierarchy; and the level-1 Galerkin summand D^-1 A_nm to the last bit."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import meshes
import solve_ref_mg
from rdcfes_amd import synth

ROOT = Path(__file__).resolve().parent.parent
LISTS = {"agg": (0, np.int32), "mptr": (1, np.int64), "member": (2, np.int32), "bptr": (3, np.int64), "bcol": (4, np.int32),
         "cptr": (5, np.int64), "cidx": (6, np.int32), "cnode": (7, np.int32)}


@pytest.fixture(scope="module")
def lib():
    out = ROOT / "tests" / "_build" / "libhost_solve_mg_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_solve_mg_shim.cpp"
    hdr = ROOT / "rdcfes_amd" / "csrc" / "rdc_solve.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        str(src), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.shim_mg_build.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
    lib.shim_mg_list.restype = C.c_int64
    lib.shim_mg_list.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.shim_scaled_block.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _patterns():
    conn, xyz = synth.kuhn_tet_mesh(8, order="random")
    yield "pihna_kuhn8", 4, conn, xyz.shape[0], 5
    conn, xyz = synth.hex_mesh(6, jitter=0.1, order="random")
    yield "hcc_hex", 8, conn, xyz.shape[0], 3
    conn, xyz = meshes.hub(max(meshes.HUB_TETS.values()))
    yield "pihna_hub", 4, conn, xyz.shape[0], 5
    conn, xyz = meshes.hydrogel()
    yield "pihna_hydrogel", 4, conn, xyz.shape[0], 5


def _steps(lib, bptr, bcol):
    bptr, bcol = np.ascontiguousarray(bptr, dtype=np.int64), np.ascontiguousarray(bcol, dtype=np.int32)
    n_steps = lib.shim_mg_build(bptr.size - 1, bptr.ctypes.data, bcol.ctypes.data)
    assert n_steps >= 0
    out = []
    for l in range(n_steps):
        st = dict(n_fine=lib.shim_mg_list(l, 100, None), n=lib.shim_mg_list(l, 101, None), n_pass1=lib.shim_mg_list(l, 102, None))
        for name, (which, dt) in LISTS.items():
            a = np.empty(lib.shim_mg_list(l, which, None), dtype=dt)
            assert lib.shim_mg_list(l, which, a.ctypes.data) == a.size
            st[name] = a
        out.append(st)
    return out


def test_constants_are_those_of_the_yardstick(lib):
    c = (C.c_int * 6)()
    assert lib.shim_mg_constants(c) == 6
    assert list(c) == [solve_ref_mg.AGG_CAP, solve_ref_mg.MIN_FREE, solve_ref_mg.COARSEST_NODES, solve_ref_mg.MAX_LEVELS,
                       solve_ref_mg.COARSEST_SWEEPS, round(1000 * solve_ref_mg.OMEGA)]
    assert list(c) == [8, 3, 40, 10, 8, 600]


@pytest.mark.parametrize("case", list(_patterns()), ids=lambda c: c[0])
def test_hierarchy_against_numpy(oracle, lib, case):
    name, et, conn, nn, nv = case
    _, _, bptr, bcol = oracle.build_pattern(et, conn, nn, nn, nv)
    got, ref = _steps(lib, bptr, bcol), solve_ref_mg.pattern_hierarchy(bptr.astype(np.int64), bcol.astype(np.int32))
    print(name, "levels (nodes, blocks):", [(nn, bcol.size)] + [(st["n"], st["bcol"].size) for st in got])
    assert len(got) == len(ref) >= 2
    fb, fc = bptr.astype(np.int64), bcol.astype(np.int32)
    for st, rf in zip(got, ref):
        n_fine, n = fb.size - 1, st["n"]
        assert (st["n_fine"], n, st["n_pass1"]) == (n_fine, rf["n"], rf["n_pass1"])
        for key in ("agg", "bptr", "bcol", "cptr", "cidx"):
            np.testing.assert_array_equal(st[key], rf[key], err_msg=f"{name} {key}")
        # every node in exactly one aggregate; the member lists are its inverse, ascending
        assert st["agg"].min() == 0 and st["agg"].max() == n - 1
        np.testing.assert_array_equal(np.sort(st["member"]), np.arange(n_fine))
        np.testing.assert_array_equal(np.diff(st["mptr"]), np.bincount(st["agg"], minlength=n))
        for i in range(n):
            m = st["member"][st["mptr"][i]:st["mptr"][i + 1]]
            assert m.size >= 1 and np.all(st["agg"][m] == i) and np.all(np.diff(m) > 0)
            assert np.all(np.diff(st["bcol"][st["bptr"][i]:st["bptr"][i + 1]]) > 0)
        assert rf["pass1_sizes"].max() <= solve_ref_mg.AGG_CAP        # of the aggregation the compiled code reproduces exactly
        # every coarse block has a contribution, every fine block contributes exactly once, to the block of its aggregates
        assert st["cptr"][0] == 0 and st["cptr"][-1] == fc.size and np.diff(st["cptr"]).min() >= 1
        np.testing.assert_array_equal(np.sort(st["cidx"]), np.arange(fc.size))
        rows = np.repeat(np.arange(n_fine), np.diff(fb))
        np.testing.assert_array_equal(st["cnode"], rows[st["cidx"]])
        cb = np.repeat(np.arange(st["bcol"].size), np.diff(st["cptr"]))
        crow = np.repeat(np.arange(n), np.diff(st["bptr"]))
        np.testing.assert_array_equal(crow[cb], st["agg"][rows[st["cidx"]]])
        np.testing.assert_array_equal(st["bcol"][cb], st["agg"][fc[st["cidx"]]])
        for c in range(st["bcol"].size):
            assert np.all(np.diff(st["cidx"][st["cptr"][c]:st["cptr"][c + 1]]) > 0)
        fb, fc = st["bptr"], st["bcol"]
    assert fb.size - 1 <= solve_ref_mg.COARSEST_NODES or len(got) + 1 == solve_ref_mg.MAX_LEVELS
    if name == "pihna_hub":
        assert np.diff(bptr).max() >= 740 and np.bincount(got[0]["agg"]).max() > 100      # the giant aggregate of the hub


@pytest.mark.parametrize("nv", [3, 5])
def test_galerkin_summand_to_the_last_bit(lib, nv):
    rng = np.random.default_rng(nv)
    for scale in (1.0, 1e-7, 1e9):
        d = rng.standard_normal((nv, nv)) * scale
        a = rng.standard_normal((nv, nv)) / 3.0
        out = np.empty((nv, nv))
        assert lib.shim_scaled_block(nv, d.ctypes.data, a.ctypes.data, out.ctypes.data) == 0
        ref = solve_ref_mg.scaled_blocks(d[None], a[None])[0]
        assert out.tobytes() == ref.tobytes()
        assert np.abs(out - d @ a).max() <= 4 * nv * np.finfo(np.float64).eps * (np.abs(d) @ np.abs(a)).max()
