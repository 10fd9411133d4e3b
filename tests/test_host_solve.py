"""CPU build of rdcfes_amd/csrc/rdc_solve.h (tests/host_solve_shim.cpp): the block inverse of the Jacobi preconditioner
against numpy on the diagonal blocks of oracle-assembled matrices, the index arithmetic of the block pattern against the
oracle's scalar col_idx, and the Python surface of the solver (struct sizes, methods) -- none of which exists without
the device-resident solve."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sps

import meshes
import solve_ref
import solve_systems
from rdcfes_amd import synth

ROOT = Path(__file__).resolve().parent.parent
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def shim():
    out = ROOT / "tests" / "_build" / "libhost_solve_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_solve_shim.cpp"
    hdr = ROOT / "rdcfes_amd" / "csrc" / "rdc_solve.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", str(src),
                        "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.shim_expand_pattern.restype = C.c_int64
    return lib


def _inv(lib, d):
    m = np.ascontiguousarray(d, dtype=np.float64).copy()
    ok = lib.shim_block_inverse(m.shape[0], m.ctypes.data_as(C.POINTER(C.c_double)))
    return ok, m


@pytest.mark.parametrize("name", ["pihna_kuhn", "ripf_tet", "hcc_hex"])
def test_block_inverse_on_assembled_diagonal_blocks(oracle, shim, name):
    s = solve_systems.get(name)
    rp, col, val, rhs = s.oracle_assemble(oracle)
    A = sps.csr_matrix((val, col, rp), shape=(rhs.size, rhs.size))
    worst = 0.0
    for d in solve_ref.diag_blocks(A, s.nv):
        ok, di = _inv(shim, d)
        assert ok == 1
        ref = np.linalg.inv(d)
        cond = np.abs(d).sum(axis=1).max() * np.abs(ref).sum(axis=1).max()
        err = np.abs(d @ di - np.eye(s.nv)).max()
        worst = max(worst, err / (64.0 * EPS * cond))
        assert err <= 64.0 * EPS * cond
    print(f"{name}: worst ||D D^-1 - I||_max / (64 eps cond_inf) = {worst:.3f}")


@pytest.mark.parametrize("nv", [3, 5])
def test_singular_and_nan_blocks_are_reported(shim, nv):
    rng = np.random.default_rng(nv)
    d = rng.integers(-4, 5, (nv, nv)).astype(np.float64) + 10.0 * np.eye(nv)
    assert _inv(shim, d)[0] == 1
    sing = d.copy()
    sing[nv - 1] = sing[0]                      # two equal rows of small integers: the elimination meets an exact zero
    assert _inv(shim, sing)[0] == 0
    assert _inv(shim, np.zeros((nv, nv)))[0] == 0
    bad = d.copy()
    bad[1, 1] = np.nan
    assert _inv(shim, bad)[0] == 0
    bad[1, 1] = np.inf
    assert _inv(shim, bad)[0] == 0
    # the preconditioner leaves the identity behind for a block it reports, in all three modes
    for precond in (2, 1):
        m = np.zeros((nv, nv))
        assert shim.shim_precond_block(nv, m.ctypes.data_as(C.POINTER(C.c_double)), precond) == 0
        np.testing.assert_array_equal(m, np.eye(nv))
    m = d.copy()
    assert shim.shim_precond_block(nv, m.ctypes.data_as(C.POINTER(C.c_double)), 1) == 1
    np.testing.assert_allclose(m, np.diag(1.0 / np.diag(d)), rtol=4 * EPS)
    m = d.copy()
    assert shim.shim_precond_block(nv, m.ctypes.data_as(C.POINTER(C.c_double)), 0) == 1
    np.testing.assert_array_equal(m, np.eye(nv))


def _pattern_cases():
    conn, xyz = synth.kuhn_tet_mesh(5, order="random")
    yield "kuhn", 4, conn, xyz.shape[0], 5
    conn, xyz = synth.hex_mesh(5, jitter=0.1, order="random")
    yield "hex8", 8, conn, xyz.shape[0], 3
    conn, xyz = meshes.hydrogel()
    yield "hydrogel", 4, conn, xyz.shape[0], 5


def test_offsets_reproduce_the_oracle_col_idx(oracle, shim):
    for name, et, conn, nn, nv in _pattern_cases():
        rp, col, bptr, bcol = oracle.build_pattern(et, conn, nn, nn, nv)
        out = np.full(col.size, -1, dtype=np.int32)
        n = shim.shim_expand_pattern(nv, C.c_int64(nn), bptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                     bcol.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int64(col.size),
                                     out.ctypes.data_as(C.POINTER(C.c_int32)))
        assert n == col.size, name
        np.testing.assert_array_equal(out, col, err_msg=name)
        kd = np.empty(nn, dtype=np.int64)
        shim.shim_diag_blocks(C.c_int64(nn), bptr.ctypes.data_as(C.POINTER(C.c_int64)), bcol.ctypes.data_as(C.POINTER(C.c_int32)),
                              kd.ctypes.data_as(C.POINTER(C.c_int64)))
        assert np.all(kd >= 0), name
        np.testing.assert_array_equal(bcol[bptr[:-1] + kd], np.arange(nn), err_msg=name)


def test_python_surface_of_the_solver():
    import rdcfes_amd
    from rdcfes_amd import AssemblyContext
    assert C.sizeof(rdcfes_amd.SolveParams) == 32 and C.sizeof(rdcfes_amd.SolveInfo) == 56
    for m in ("csr_matvec", "csr_matvec_device", "solve"):
        assert callable(getattr(AssemblyContext, m))
    assert (rdcfes_amd.PRECOND_NONE, rdcfes_amd.PRECOND_JACOBI, rdcfes_amd.PRECOND_BLOCK_JACOBI) == (0, 1, 2)
    assert rdcfes_amd.SOLVE_NOT_FINITE == 4
