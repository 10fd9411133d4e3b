"""CPU build of the GMRES functions of rdcfes_amd/csrc/rdc_solve.h as compiled by g++ (tests/host_solve_gmres_shim.cpp): the Givens
step of a column (gmres_givens_step) and the back substitution (gmres_back_substitute), which the device runs in k_gmres_finalize
and k_gmres_solve_y, against numpy.linalg.lstsq; and the one statement of the layout of the GMRES state (gmres_carve)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
EPS = np.finfo(np.float64).eps
PARTS = ["V", "H", "R", "cs", "sn", "g", "y", "hpass", "scal", "partials", "rec"]


@pytest.fixture(scope="module")
def lib():
    out = ROOT / "tests" / "_build" / "libhost_solve_gmres_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_solve_gmres_shim.cpp"
    hdr = ROOT / "rdcfes_amd" / "csrc" / "rdc_solve.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        str(src), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.shim_gmres_lstsq.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_double] + [C.c_void_p] * 8
    lib.shim_gmres_carve.restype = None
    lib.shim_gmres_carve.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_void_p]
    return lib


def _const(lib):
    names = ["MAX_RESTART", "DEFAULT_RESTART", "NOT_FINITE", "HAPPY", "SINGULAR", "SCALARS", "REC_BYTES", "VEC_PER_BLOCK"]
    return {k: lib.shim_gmres_constants(i) for i, k in enumerate(names)}


def _lstsq(lib, H, beta, k=None):
    """H: (m + 1) x m raw Hessenberg matrix -> dict(taken, y, flags, y_ok, est, R, g)"""
    m = H.shape[1]
    k = m if k is None else k
    Hc = np.asfortranarray(H, dtype=np.float64)
    R = np.full((m + 1, m), 7.0, order="F")
    cs, sn, g, y = np.full(m, 7.0), np.full(m, 7.0), np.full(m + 1, 7.0), np.full(m, 7.0)
    flags = np.zeros(m, dtype=np.int32)
    y_ok, est = C.c_int(), C.c_double()
    p = lambda a: a.ctypes.data   # noqa: E731
    taken = lib.shim_gmres_lstsq(m, k, p(Hc), beta, p(R), p(cs), p(sn), p(g), p(y), p(flags), C.addressof(y_ok), C.addressof(est))
    return dict(taken=taken, y=y[:taken], flags=flags, y_ok=bool(y_ok.value), est=est.value, R=R, g=g, cs=cs, sn=sn)


def _hessenberg(rng, m):
    H = np.triu(rng.standard_normal((m + 1, m)), -1)
    H[np.arange(1, m + 1), np.arange(m)] = np.abs(H[np.arange(1, m + 1), np.arange(m)]) + 0.1    # a norm: positive
    return H + np.vstack([3.0 * np.eye(m), np.zeros((1, m))])


@pytest.mark.parametrize("m", [1, 2, 30, 128])
def test_least_squares_against_numpy(lib, m):
    rng = np.random.default_rng(m)
    H, beta = _hessenberg(rng, m), 2.5
    out = _lstsq(lib, H, beta)
    rhs = np.zeros(m + 1)
    rhs[0] = beta
    want, *_ = np.linalg.lstsq(H, rhs, rcond=None)
    cond = np.linalg.cond(H)
    assert out["taken"] == m and out["y_ok"] and not out["flags"].any()
    assert np.linalg.norm(out["y"] - want) <= 64 * m * EPS * cond * np.linalg.norm(want)
    assert abs(out["est"] - np.linalg.norm(rhs - H @ want)) <= 64 * m * EPS * beta      # |g_m| is the least-squares residual
    assert np.all(out["R"][np.arange(1, m + 1), np.arange(m)] == 0.0)                   # the rotations emptied the subdiagonal ...
    below = np.arange(m + 1)[:, None] > np.arange(m)[None, :] + 1
    assert np.all(out["R"][below] == 7.0)                                               # ... and nothing below it was touched
    # every leading k: the estimate of step k is the residual of the k-column problem (what ends a cycle early)
    for k in sorted({1, max(1, m // 2)}):
        part = _lstsq(lib, H, beta, k)
        w, *_ = np.linalg.lstsq(H[:k + 1, :k], rhs[:k + 1], rcond=None)
        assert part["taken"] == k and np.linalg.norm(part["y"] - w) <= 64 * m * EPS * np.linalg.cond(H[:k + 1, :k]) * np.linalg.norm(w)
        assert abs(part["est"] - np.linalg.norm(rhs[:k + 1] - H[:k + 1, :k] @ w)) <= 64 * m * EPS * beta


def test_zero_subdiagonal_is_an_exact_solve(lib):
    """h_{j+1,j} = 0 (the Krylov space is exhausted): the column is taken, the estimate is exactly 0, y solves the square system"""
    rng = np.random.default_rng(9)
    m, k = 6, 4
    H = _hessenberg(rng, m)
    H[k, k - 1] = 0.0
    out = _lstsq(lib, H, 1.5, k)
    want = np.linalg.solve(H[:k, :k], np.r_[1.5, np.zeros(k - 1)])
    assert out["taken"] == k and out["y_ok"] and out["est"] == 0.0 and out["sn"][k - 1] == 0.0
    assert np.linalg.norm(out["y"] - want) <= 64 * EPS * np.linalg.cond(H[:k, :k]) * np.linalg.norm(want)


def test_a_zero_column_is_singular_and_not_taken(lib):
    c = _const(lib)
    H = _hessenberg(np.random.default_rng(2), 4)
    H[:, 0] = 0.0
    out = _lstsq(lib, H, 1.0)
    assert out["taken"] == 0 and out["flags"][0] == c["SINGULAR"]
    assert out["g"][0] == 1.0 and np.all(out["g"][1:] == 7.0) and np.all(out["cs"] == 7.0)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("row", [0, 2, 3])
def test_a_non_finite_entry_is_flagged_and_not_propagated(lib, bad, row):
    c = _const(lib)
    m, j = 5, 2
    H = _hessenberg(np.random.default_rng(3), m)
    clean = _lstsq(lib, H, 1.0, j)
    H[row, j] = bad                       # rows 0 .. j + 1 of column j are what the step reads
    out = _lstsq(lib, H, 1.0)
    assert out["taken"] == j and out["flags"][j] == c["NOT_FINITE"] and out["y_ok"]
    for key in ("g", "cs", "sn", "R"):    # what the first j columns left is untouched, and nothing non-finite was stored
        assert out[key].tobytes() == clean[key].tobytes(), key
    assert np.array_equal(out["y"], clean["y"]) and np.all(np.isfinite(out["y"]))
    assert np.all(np.isfinite(out["g"])) and np.all(np.isfinite(out["R"]))


def test_back_substitution_reports_an_overflow(lib):
    H = np.array([[1e-300, 0.0], [1e-300, 1.0], [0.0, 1.0]])
    out = _lstsq(lib, H, 1e300)
    assert out["taken"] == 2 and not out["y_ok"]


@pytest.mark.parametrize("nvar,n_owned,restart", [(3, 343, 30), (5, 729, 30), (5, 729, 1), (3, 343, 128), (5, 0, 30), (3, 1, 2),
                                                  (5, 1685159, 30), (5, 2 ** 27, 60)])
def test_layout(lib, nvar, n_owned, restart):
    c = _const(lib)
    out = np.zeros(16, dtype=np.int64)
    lib.shim_gmres_carve(nvar, n_owned, restart, out.ctypes.data)
    off = dict(zip(PARTS, out[:11].tolist()))
    nbytes, basis_bytes, partial_count, vec_blocks, stride = out[11:].tolist()
    m, n = restart, n_owned * nvar
    assert stride == max(n, 1) and vec_blocks == -(-n // c["VEC_PER_BLOCK"])
    size = dict(V=(m + 1) * stride, H=(m + 1) * m, R=(m + 1) * m, cs=m, sn=m, g=m + 1, y=m, hpass=m + 1, scal=c["SCALARS"],
                partials=partial_count, rec=c["REC_BYTES"] // 8)
    assert c["REC_BYTES"] % 8 == 0 and c["SCALARS"] >= 3
    # no overlap: the parts in address order tile the allocation exactly, and bytes is what they add up to
    at = 0
    for name in sorted(PARTS, key=lambda k: off[k]):
        assert off[name] == at, (name, off)
        at += size[name]
    assert nbytes == 8 * at == 8 * sum(size.values())
    assert basis_bytes == 8 * (m + 1) * stride
    # the partials cover every step: step j < m leaves j + 2 components of vec_blocks entries each
    assert partial_count >= (m + 1) * vec_blocks and all((j + 2) * vec_blocks <= partial_count for j in range(m))


def test_constants(lib):
    c = _const(lib)
    assert c["MAX_RESTART"] == 128 and c["DEFAULT_RESTART"] == 30
    assert len({c["NOT_FINITE"], c["HAPPY"], c["SINGULAR"]}) == 3
