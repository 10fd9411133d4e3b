"""CPU build of the block ILU(0) functions of rdcfes_amd/csrc/rdc_solve.h as compiled by g++ (tests/host_solve_ilu_shim.cpp):
the host builder of the lists (ilu_build: colours, rows in elimination order, lower counts), the index arithmetic of the private
layout (ilu_value_offset, ilu_find), the factor step of a node (ilu_factor_node, driven node after node by ilu_factor_host) and
the placement (ilu_place), held against the numpy yardstick tests/solve_ref_ilu.py on oracle-assembled systems: K(8) (nvar 5,
15-block rows), the HEX8 mesh (nvar 3, 27-block rows) and the hub mesh (one row of 740 blocks)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sps

import solve_ref_ilu
import solve_ref_mg_gs
import solve_systems

ROOT = Path(__file__).resolve().parent.parent
LISTS = {"colour": (0, np.int32), "cptr": (1, np.int64), "nodes": (2, np.int32), "pcol": (3, np.int32), "nlow": (4, np.int32)}
EPS = np.finfo(np.float64).eps
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    out = ROOT / "tests" / "_build" / "libhost_solve_ilu_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_solve_ilu_shim.cpp"
    hdr = ROOT / "rdcfes_amd" / "csrc" / "rdc_solve.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        str(src), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.shim_ilu_build.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.shim_ilu_list.restype = C.c_int64
    lib.shim_ilu_list.argtypes = [C.c_int, C.c_void_p]
    lib.shim_ilu_offsets.restype = None
    lib.shim_ilu_offsets.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.shim_ilu_find.restype = C.c_int64
    lib.shim_ilu_find.argtypes = [C.c_int64, C.c_int32]
    lib.shim_ilu_factor.restype = C.c_int64
    lib.shim_ilu_factor.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.shim_ilu_place.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    return lib


def _system(oracle, name):
    """(nv, A, FP64 yardstick factor, extended-precision yardstick factor) of an oracle-assembled system, once"""
    if name not in _CACHE:
        s = solve_systems.get(name)
        rp, col, val, rhs = s.oracle_assemble(oracle)
        A = sps.csr_matrix((val, col, rp), shape=(rhs.size, rhs.size))
        _CACHE[name] = (s.nv, A, solve_ref_ilu.Factor(A, s.nv), solve_ref_ilu.Factor(A, s.nv, dtype=np.longdouble))
    return _CACHE[name]


def _build(lib, bptr, bcol):
    where = C.c_int64(-1)
    rc = lib.shim_ilu_build(bptr.size - 1, bptr.ctypes.data, bcol.ctypes.data, C.byref(where))
    out = {}
    for name, (which, dt) in LISTS.items():
        a = np.empty(lib.shim_ilu_list(which, None), dtype=dt)
        assert lib.shim_ilu_list(which, a.ctypes.data) == a.size
        out[name] = a
    return rc, where.value, out


def _rel(a, ref):
    d = np.asarray(a, dtype=np.longdouble) - ref
    return float(np.sqrt(d @ d) / np.sqrt(ref @ ref)), float(np.abs(d).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", ["pihna_kuhn", "hcc_hex", "pihna_hub"])
def test_lists_layout_and_factor_against_the_yardstick(oracle, lib, name):
    nv, A, f, fl = _system(oracle, name)
    bptr, bcol, n = f.bptr, f.bcol, f.n
    rc, _, got = _build(lib, bptr, bcol)
    assert rc == 0
    # the lists: greedy colours, every row in (colour, node id) order, the lower blocks counted
    col, cptr, nodes = solve_ref_mg_gs.colour(bptr, bcol)
    np.testing.assert_array_equal(got["colour"], col)
    np.testing.assert_array_equal(got["cptr"], cptr)
    np.testing.assert_array_equal(got["nodes"], nodes)
    np.testing.assert_array_equal(got["nodes"], f.order)
    for i in range(n):
        row = got["pcol"][bptr[i]:bptr[i + 1]]
        want = np.concatenate([bcol[f.lower[i]], [i], bcol[f.upper[i]]])
        np.testing.assert_array_equal(row, want, err_msg=f"{name} node {i}")
        assert got["nlow"][i] == f.lower[i].size and row[got["nlow"][i]] == i
    if name == "pihna_hub":
        assert np.diff(bptr).max() >= 740
    # the private layout: a bijection onto the node's own nvar^2 * len values, three contiguous runs, rows of a run contiguous
    nblk = int(bptr[-1])
    off, find = np.empty(nblk * nv * nv, dtype=np.int64), np.empty(nblk, dtype=np.int64)
    lib.shim_ilu_offsets(nv, off.ctypes.data, find.ctypes.data)
    np.testing.assert_array_equal(np.sort(off), np.arange(nblk * nv * nv))
    np.testing.assert_array_equal(find, np.arange(nblk) - np.repeat(bptr[:-1], np.diff(bptr)))
    off = off.reshape(nblk, nv, nv)
    for i in (0, n // 2, n - 1, int(np.argmax(np.diff(bptr)))):
        b0, ln, nl = int(bptr[i]), int(bptr[i + 1] - bptr[i]), int(got["nlow"][i])
        o = off[b0:b0 + ln]
        assert o.min() == nv * nv * b0 and o.max() == nv * nv * (b0 + ln) - 1
        lower, diag, upper = o[:nl], o[nl], o[nl + 1:]
        np.testing.assert_array_equal(lower.transpose(1, 0, 2).reshape(-1), nv * nv * b0 + np.arange(nl * nv * nv))
        np.testing.assert_array_equal(diag.reshape(-1), nv * nv * (b0 + nl) + np.arange(nv * nv))
        np.testing.assert_array_equal(upper.transpose(1, 0, 2).reshape(-1), nv * nv * (b0 + nl + 1) + np.arange((ln - nl - 1) * nv * nv))
    # a column the row does not have
    far = next(j for j in range(n) if j not in set(bcol[bptr[0]:bptr[1]].tolist()))
    assert lib.shim_ilu_find(0, far) == -1
    # the factor: from the yardstick's own FP64 A^, against the extended-precision factor; bound = 64 x the FP64 yardstick's own error
    ahat = solve_ref_ilu.scaled_values(A, nv)
    val, uinv = np.empty(ahat.size), np.empty((n, nv, nv))
    assert lib.shim_ilu_factor(nv, ahat.ctypes.data, val.ctypes.data, uinv.ctypes.data) == 0
    noise_f, noise_u = max(_rel(f.values(), fl.values())), max(_rel(f.Uinv.reshape(-1), fl.Uinv.reshape(-1)))
    err_f, err_u = max(_rel(val, fl.values())), max(_rel(uinv.reshape(-1), fl.Uinv.reshape(-1)))
    print(f"{name}: colours {cptr.size - 1}; factor error {err_f:.2e} (numpy FP64 {noise_f:.2e}), U_ii^-1 error {err_u:.2e} (numpy FP64 {noise_u:.2e})")
    assert err_f <= 64.0 * max(noise_f, 16.0 * EPS)
    assert err_u <= 64.0 * max(noise_u, 16.0 * EPS)
    # the placement: measured, then placed into arenas of exactly the measured sizes; aligned, in bounds, disjoint, lists arrived
    nbytes, offs = np.zeros(2, dtype=np.int64), np.zeros(8, dtype=np.int64)
    assert lib.shim_ilu_place(nv, None, 0, None, 0, nbytes.ctypes.data, offs.ctypes.data) == 0
    assert np.all(nbytes % 256 == 0) and nbytes[1] >= 8 * (nblk * nv * nv + n * nv * nv + 2 * n * nv) and nbytes[0] >= 4 * (nblk + 3 * n)
    idx, arena = np.full(nbytes[0], 0x5A, dtype=np.uint8), np.zeros(nbytes[1], dtype=np.uint8)
    assert lib.shim_ilu_place(nv, idx.ctypes.data, nbytes[0] - 1, arena.ctypes.data, nbytes[1], nbytes.ctypes.data, offs.ctypes.data) == -1
    assert lib.shim_ilu_place(nv, idx.ctypes.data, nbytes[0], arena.ctypes.data, nbytes[1], nbytes.ctypes.data, offs.ctypes.data) == 0
    for at, a in zip(offs[:4], (got["pcol"], got["nlow"], got["colour"], got["nodes"])):
        assert at % 256 == 0 and idx[at:at + a.nbytes].tobytes() == a.tobytes()
    sizes = [8 * nblk * nv * nv, 8 * n * nv * nv, 8 * n * nv, 8 * n * nv]
    spans = sorted((int(at), int(at) + sz) for at, sz in zip(offs[4:], sizes))
    assert all(at % 256 == 0 for at, _ in spans) and spans[-1][1] <= nbytes[1]
    assert all(e0 <= s1 for (_, e0), (s1, _) in zip(spans, spans[1:]))


def test_exactly_singular_schur_pivot_is_a_bad_block(lib):
    """two coupled nodes, one unknown each: A^ = [[1, 2], [3, 6]], so U_11 = 6 - 3 * 2 = 0 exactly; with 6.5 in its place the factor
    is L_10 = 3, U_11 = 0.5"""
    bptr, bcol = np.array([0, 2, 4], dtype=np.int64), np.array([0, 1, 0, 1], dtype=np.int32)
    rc, _, got = _build(lib, bptr, bcol)
    assert rc == 0 and got["colour"].tolist() == [0, 1] and got["nlow"].tolist() == [0, 1]
    val, uinv = np.empty(4), np.empty(2)
    a = np.array([1.0, 2.0, 3.0, 6.0])
    assert lib.shim_ilu_factor(1, a.ctypes.data, val.ctypes.data, uinv.ctypes.data) == 1
    assert uinv.tolist() == [1.0, 1.0]                     # the identity where the pivot is bad: an apply stays harmless
    a[3] = 6.5
    assert lib.shim_ilu_factor(1, a.ctypes.data, val.ctypes.data, uinv.ctypes.data) == 0
    assert val.tolist() == [1.0, 2.0, 3.0, 0.5] and uinv.tolist() == [1.0, 2.0]
    a[0] = np.nan                                           # a non-finite pivot counts as well; its inverse is the identity
    assert lib.shim_ilu_factor(1, a.ctypes.data, val.ctypes.data, uinv.ctypes.data) == 1
    assert uinv.tolist() == [1.0, 2.0]


def test_builder_refuses_what_it_cannot_order(lib):
    bptr, bcol = np.array([0, 2, 3], dtype=np.int64), np.array([0, 1, 1], dtype=np.int32)      # block (0, 1) without (1, 0)
    assert _build(lib, bptr, bcol)[0] == 1                                                      # node 1 does not see node 0: both take colour 0
    bptr, bcol = np.array([0, 1, 3], dtype=np.int64), np.array([0, 0, 1], dtype=np.int32)      # block (1, 0) without (0, 1): the later
    rc, _, got = _build(lib, bptr, bcol)                                                        # node sees the earlier one, the colours differ
    assert rc == 0 and got["colour"].tolist() == [0, 1]
    bptr, bcol = np.array([0, 1, 3], dtype=np.int64), np.array([1, 0, 1], dtype=np.int32)      # node 0 has no diagonal block
    rc, where, _ = _build(lib, bptr, bcol)
    assert (rc, where) == (2, 0)
    bptr, bcol = np.array([0, 2, 4], dtype=np.int64), np.array([0, 2, 0, 1], dtype=np.int32)   # a column that is no row
    assert _build(lib, bptr, bcol)[0] == 2
