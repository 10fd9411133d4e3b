"""CPU build of the functions of the fp32 copy of the block ILU(0) factor in rdcfes_amd/csrc/rdc_solve.h as compiled by g++
(tests/host_solve_ilu_f32_shim.cpp): the layout (ilu_f32_offset, ilu_f32_node_floats, ilu_f32_offsets), its placement
(ilu_place_f32), and a replay of what a solve with "ilu_factor_bits" = 32 does -- the FP64 factor through ilu_factor_node, the
rounding of its lower and upper blocks, the forward and the backward sweep -- through those offsets, held against the numpy
yardstick tests/solve_ref_ilu_f32.py: the numpy sweeps of the replay's OWN FP64 factor, rounded by numpy, in extended precision.
Bound: ld.bound(64, noise), noise = numpy's FP64 evaluation of the same sweeps against the extended-precision one.

Systems: a block-tridiagonal and an arrow matrix for nvar 1, 3 and 5; K(3) (64 nodes, nvar 5) whole and as the three ranks of a
split, whose patterns have ghost columns.  tests/host_solve_ilu_f32_main.cpp runs the same functions as a stand-alone program under
AddressSanitizer and UBSan."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import solve_ref_dist
import solve_ref_ilu
import solve_ref_ilu_f32
import solve_ref_mg
import solve_ref_mg_ld as ld
from test_solve_ref_ilu import _arrow, _block_tridiagonal

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "rdcfes_amd" / "csrc" / "rdc_solve.h"
MARGIN = 64.0


@pytest.fixture(scope="module")
def lib():
    out = ROOT / "tests" / "_build" / "libhost_solve_ilu_f32_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_solve_ilu_f32_shim.cpp"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        str(src), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.shim_f32_build.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    lib.shim_f32_lists.restype = None
    lib.shim_f32_lists.argtypes = [C.c_void_p, C.c_void_p]
    lib.shim_f32_offsets.restype = None
    lib.shim_f32_offsets.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.shim_f32_factor.restype = C.c_int64
    lib.shim_f32_factor.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.shim_f32_values.restype = C.c_int64
    lib.shim_f32_values.argtypes = [C.c_void_p]
    lib.shim_f32_apply.restype = None
    lib.shim_f32_apply.argtypes = [C.c_void_p, C.c_void_p]
    lib.shim_f32_place.restype = C.c_int64
    lib.shim_f32_place.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    return lib


def _check(lib, A, nv, n, label):
    """A: [n * nv][n_local * nv], columns >= n * nv are ghost columns.  Layout, placement, rounding and one apply."""
    bptr, bcol, _ = solve_ref_mg.block_pattern(A, nv)
    ghosts = int(bcol.max()) >= n
    sq = A[:, :n * nv].tocsr()
    f = solve_ref_ilu.Factor(sq, nv)
    assert lib.shim_f32_build(n, bptr.ctypes.data, bcol.ctypes.data, 1 if ghosts else 0) == 0
    nown, nlow = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    lib.shim_f32_lists(nown.ctypes.data, nlow.ctypes.data)
    np.testing.assert_array_equal(nown, np.diff(f.bptr))
    np.testing.assert_array_equal(nlow, [lo.size for lo in f.lower])
    # the layout: every (a, p != nlow, b) of an owned position exactly once, no slot for a diagonal or a ghost block, every row of
    # a run at a multiple of 4 floats, a node's floats = nvar * (padded lower row + padded upper row)
    nblk = int(bptr[-1])
    foff, off, floats = np.empty(n + 1, dtype=np.int64), np.empty(nblk * nv * nv, dtype=np.int64), np.empty(n, dtype=np.int64)
    lib.shim_f32_offsets(nv, foff.ctypes.data, off.ctypes.data, floats.ctypes.data)
    off = off.reshape(nblk, nv, nv)
    pad4 = lambda k: (k + 3) // 4 * 4   # noqa: E731
    want_floats = nv * (pad4(nv * nlow.astype(np.int64)) + pad4(nv * (nown.astype(np.int64) - nlow - 1)))
    np.testing.assert_array_equal(floats, want_floats)
    np.testing.assert_array_equal(foff, np.concatenate([[0], np.cumsum(want_floats)]))
    used = off[off >= 0]
    assert used.size == nv * nv * (int(nown.sum()) - n) and np.unique(used).size == used.size
    for i in range(n):
        b0, ln, own, nl = int(bptr[i]), int(bptr[i + 1] - bptr[i]), int(nown[i]), int(nlow[i])
        o = off[b0:b0 + ln]
        assert np.all(o[nl] == -1) and np.all(o[own:] == -1), f"{label} node {i}: a diagonal or a ghost block has a slot"
        mine = np.delete(o[:own], nl, axis=0)
        if mine.size:
            assert mine.min() >= foff[i] and mine.max() < foff[i + 1]
        lower, upper = o[:nl], o[nl + 1:own]
        for run, start in ((lower, foff[i]), (upper, foff[i] + nv * pad4(nv * nl))):
            if not run.size:
                continue
            stride = pad4(nv * run.shape[0])
            for a in range(nv):   # row a of the run: contiguous, ascending in (block, b), at a multiple of 4 floats
                row = run[:, a, :].reshape(-1)
                assert row[0] == start + a * stride and row[0] % 4 == 0
                np.testing.assert_array_equal(row, row[0] + np.arange(row.size))
    # the placement: measured, then into an arena of exactly that size
    at = np.zeros(2, dtype=np.int64)
    nbytes = lib.shim_f32_place(nv, None, 0, at.ctypes.data)
    assert nbytes % 256 == 0 and nbytes >= 8 * (n + 1) + 4 * int(foff[-1])
    arena = np.zeros(nbytes + 256, dtype=np.uint8)
    base = arena.ctypes.data + (-arena.ctypes.data) % 256
    assert lib.shim_f32_place(nv, base, nbytes - 1, at.ctypes.data) == -1
    assert lib.shim_f32_place(nv, base, nbytes, at.ctypes.data) == nbytes
    assert at[0] == 0 and at[1] % 256 == 0 and at[1] >= 8 * (n + 1) and at[1] + 4 * max(int(foff[-1]), 1) <= nbytes
    lo = base - arena.ctypes.data
    assert arena[lo:lo + 8 * (n + 1)].tobytes() == foff.tobytes()
    # the replay: FP64 factor, rounding (padding zero, every other float written), one apply per probe vector
    ahat = solve_ref_ilu.scaled_values(sq, nv)
    val, uinv, overflow = np.empty(ahat.size), np.empty((n, nv, nv)), C.c_int64(-1)
    assert lib.shim_f32_factor(nv, ahat.ctypes.data, val.ctypes.data, uinv.ctypes.data, C.byref(overflow)) == 0 and overflow.value == 0
    v32 = np.empty(lib.shim_f32_values(None), dtype=np.float32)
    assert v32.size == foff[-1] and lib.shim_f32_values(v32.ctypes.data) == v32.size
    assert not np.any(np.isnan(v32))
    padding = np.ones(v32.size, dtype=bool)
    padding[used] = False
    assert np.all(v32[padding] == 0.0) and np.count_nonzero(padding) == v32.size - used.size
    blocks = solve_ref_ilu_f32.blocks_of(f.bptr, val, nv)           # the replay's FP64 factor, bcol order
    for i in (0, n // 2, n - 1):                                      # the floats are the numpy rounding of it, where the offsets say
        row = f.bcol[f.bptr[i]:f.bptr[i + 1]]
        priv = np.concatenate([f.bcol[f.lower[i]], [i], f.bcol[f.upper[i]]])
        for p, j in enumerate(priv):
            if j != i:
                k = f.bptr[i] + int(np.searchsorted(row, j))
                assert v32[off[bptr[i] + p]].tobytes() == blocks[k].astype(np.float32).tobytes()
    g = solve_ref_ilu_f32.rounded(f, val=val, uinv=uinv.reshape(-1))
    gl = solve_ref_ilu_f32.rounded(f, dtype=np.longdouble, val=val, uinv=uinv.reshape(-1))
    plain = solve_ref_ilu_f32.unrounded(f, np.float64, val, uinv.reshape(-1))
    worst = noise = 0.0
    for y in ld.probe_vectors(n * nv, np.linspace(-1.0, 2.0, n * nv)):
        z = np.empty(n * nv)
        lib.shim_f32_apply(np.ascontiguousarray(y).ctypes.data, z.ctypes.data)
        ref = gl.apply(y)
        noise = max(noise, max(ld.rel_diff(g.apply(y), ref)))
        worst = max(worst, max(ld.rel_diff(z, ref)))
        d = float(np.linalg.norm(z - plain.apply(y)) / np.linalg.norm(z))
        assert 1e-10 <= d <= 1e-6, (label, d)                           # and it IS the rounded apply, not the FP64 one
    print(f"{label}: replayed apply error {worst:.2e} = {worst / max(noise, 16 * ld.EPS):.2f} x max(noise {noise:.2e}, 16 eps); "
          f"{int(foff[-1])} floats, {np.count_nonzero(padding)} of them padding")
    assert worst <= ld.bound(MARGIN, noise), (label, worst, noise)


@pytest.mark.parametrize("nv", [1, 3, 5])
def test_layout_rounding_and_apply_on_small_matrices(lib, nv):
    _check(lib, _block_tridiagonal(37, nv, 5 + nv), nv, 37, f"tridiagonal nvar {nv}")
    _check(lib, _arrow(23, nv, 9 + nv), nv, 23, f"arrow nvar {nv}")


def test_layout_rounding_and_apply_on_k3(oracle, lib):
    s, A, b = solve_ref_dist.global_system("pihna_kuhn3", oracle)
    assert s.xyz.shape[0] == 64
    _check(lib, A, s.nv, 64, "pihna_kuhn3")


@pytest.mark.parametrize("rank", [0, 1, 2])
def test_ghost_blocks_have_no_slot(oracle, lib, rank):
    rk = solve_ref_dist.ranks_of("pihna_kuhn3", 3, oracle)[rank]
    nv = solve_ref_dist.case("pihna_kuhn3").nv
    assert rk.A.shape[1] > rk.lp.n_owned * nv, "the case has no ghost column"
    _check(lib, rk.A, nv, rk.lp.n_owned, f"pihna_kuhn3 rank {rank} of 3")


def test_stand_alone_program_under_sanitizers():
    out = ROOT / "tests" / "_build" / "host_solve_ilu_f32_asan"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_solve_ilu_f32_main.cpp"
    deps = [src, ROOT / "tests" / "host_solve_ilu_f32_shim.cpp", HDR]
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", str(src), "-o", str(out)], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: ") and not r.stderr
