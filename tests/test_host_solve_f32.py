"""CPU build of scaled_block_f32 (rdcfes_amd/csrc/rdc_solve.h, tests/host_solve_f32_shim.cpp): one block of the fp32 copy
of D^-1 A as the set-up kernel of rdc_solve_mixed computes it -- products summed in fp64 in ascending order, one rounding
to fp32 -- against numpy's float32(Dinv @ A), its overflow report, and the Python surface of the mixed solve."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def shim():
    out = ROOT / "tests" / "_build" / "libhost_solve_f32_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_solve_f32_shim.cpp"
    hdr = ROOT / "rdcfes_amd" / "csrc" / "rdc_solve.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", str(src),
                        "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.shim_f32_row_stride.restype = C.c_longlong
    lib.shim_f32_row_stride.argtypes = [C.c_int, C.c_longlong]
    return lib


def _scaled(lib, dinv, a):
    dinv = np.ascontiguousarray(dinv, dtype=np.float64)
    a = np.ascontiguousarray(a, dtype=np.float64)
    n, nv = a.shape[0], a.shape[1]
    out = np.full(a.shape, np.nan, dtype=np.float32)
    ok = np.full(n, -1, dtype=np.int32)
    rc = lib.shim_scaled_block_f32(nv, C.c_longlong(n), dinv.ctypes.data_as(C.POINTER(C.c_double)), a.ctypes.data_as(C.POINTER(C.c_double)),
                                   out.ctypes.data_as(C.POINTER(C.c_float)), ok.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0
    return out, ok


@pytest.mark.parametrize("nv", [3, 5])
def test_against_numpy_on_random_well_conditioned_blocks(shim, nv):
    """Exact equality, except where the fp64 product lies within 4 fp64 ulp of an fp32 rounding boundary (numpy's matmul
    may sum in another order): such an entry may differ by one fp32 ulp.  At most 1 entry in 10^4 may be excused:
    a boundary every 2^29 fp64 ulp and a window of 8 make the expected share 1.5e-8."""
    rng = np.random.default_rng(2024 + nv)
    n = 20000
    d = rng.uniform(-1.0, 1.0, (n, nv, nv)) + 4.0 * np.eye(nv)          # diagonally dominant: cond_inf < 10
    dinv = np.linalg.inv(d)
    a = rng.uniform(-1.0, 1.0, (n, nv, nv)) * 10.0 ** rng.uniform(-6, 6, (n, 1, 1))
    out, ok = _scaled(shim, dinv, a)
    assert np.all(ok == 1)
    exact = np.einsum("nij,njk->nik", dinv, a)
    want = exact.astype(np.float32)
    # distance of the fp64 product to the nearest fp32 rounding boundary (midpoint of two neighbouring floats), in fp64 ulp
    up = np.nextafter(want, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(want, np.float32(-np.inf)).astype(np.float64)
    w64 = want.astype(np.float64)
    dist = np.minimum(np.abs(exact - 0.5 * (w64 + up)), np.abs(exact - 0.5 * (w64 + dn))) / np.spacing(np.abs(exact))
    near = dist <= 4.0
    differs = out != want
    print(f"nv {nv}: {int(differs.sum())} of {out.size} entries differ from numpy, {int(near.sum())} lie within 4 ulp of a boundary")
    assert near.sum() <= 1e-4 * out.size
    assert not np.any(differs & ~near)
    one_ulp = np.abs(out.astype(np.float64) - w64) <= np.spacing(np.abs(want)).astype(np.float64)
    assert np.all(one_ulp[differs])


@pytest.mark.parametrize("nv", [3, 5])
def test_overflow_underflow_and_nan(shim, nv):
    eye = np.eye(nv)[None]
    a = np.full((1, nv, nv), 2.0)
    out, ok = _scaled(shim, eye, a)
    assert ok[0] == 1 and np.all(out == np.float32(2.0))
    big = a.copy()
    big[0, 1, 2] = 3.5e38                                  # finite in fp64, above the largest float (3.4028e38)
    out, ok = _scaled(shim, eye, big)
    assert ok[0] == 0 and np.isinf(out[0, 1, 2])
    big[0, 1, 2] = -1e300
    assert _scaled(shim, eye, big)[1][0] == 0
    edge = a.copy()
    edge[0, 0, 0] = float(np.finfo(np.float32).max)        # the largest float itself fits
    out, ok = _scaled(shim, eye, edge)
    assert ok[0] == 1 and out[0, 0, 0] == np.finfo(np.float32).max
    # the scaling can bring a large entry into range, or take one out of it
    assert _scaled(shim, 1e-3 * eye, big * 0 + 1e40)[1][0] == 1
    assert _scaled(shim, 1e3 * eye, big * 0 + 1e36)[1][0] == 0
    small = a.copy()
    small[0, 0, 1], small[0, 2, 0] = 3.5e-62, 1e-40        # below the subnormal range; inside it
    out, ok = _scaled(shim, eye, small)
    assert ok[0] == 1 and out[0, 0, 1] == 0.0
    assert out[0, 2, 0] in (np.float32(0.0), np.float32(1e-40))
    for bad in (np.nan, np.inf):
        m = a.copy()
        m[0, nv - 1, 0] = bad
        assert _scaled(shim, eye, m)[1][0] == 0
        assert _scaled(shim, m, a)[1][0] == 0


def test_row_stride_of_the_fp32_copy(shim):
    for nv in (3, 5):
        for blocks in list(range(0, 40)) + [245, 740, 741]:
            s = shim.shim_f32_row_stride(nv, blocks)
            assert s % 4 == 0 and nv * blocks <= s < nv * blocks + 4


def test_python_surface_of_the_mixed_solve():
    import inspect
    import rdcfes_amd
    from rdcfes_amd import AssemblyContext, _lib
    assert C.sizeof(rdcfes_amd.SolveInfo) == 56 and rdcfes_amd.SolveInfo.matrix_bits.offset == 52
    assert rdcfes_amd.SolveInfo.matrix_bits.size == 4 and rdcfes_amd.SolveInfo.device_ms.offset == 48
    for m in ("csr_scale_f32", "csr_matvec_f32", "csr_matvec_f32_device"):
        assert callable(getattr(AssemblyContext, m))
    assert inspect.signature(AssemblyContext.solve).parameters["mixed"].default is False
    for name in ("rdc_solve_mixed", "rdc_csr_scale_f32", "rdc_csr_matvec_f32"):
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["rdc_solve_mixed"] == _lib.SIGNATURES["rdc_solve"]
