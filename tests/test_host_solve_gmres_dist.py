"""The partitioned form of the GMRES state (rdcfes_amd/csrc/rdc_solve.h, gmres_carve with n_nodes) as compiled by g++
(tests/host_solve_gmres_dist_shim.cpp): basis slots of the stride of a ghosted vector, the buffer `red` of the wide all-reduce between
the scalars and the partials, everything else where the single-partition form has it; and the stand-alone program that walks such a
state on a heap buffer of exactly its size (tests/host_solve_gmres_dist_main.cpp), which tools/asan_solve_gmres_dist.sh runs under
the sanitizers."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
PARTS = ["V", "H", "R", "cs", "sn", "g", "y", "hpass", "scal", "red", "partials", "rec"]
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"]
HDR = ROOT / "rdcfes_amd" / "csrc" / "rdc_solve.h"


def _stale(out, src):
    return not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, HDR.stat().st_mtime)


@pytest.fixture(scope="module")
def lib():
    out = ROOT / "tests" / "_build" / "libhost_solve_gmres_dist_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_solve_gmres_dist_shim.cpp"
    if _stale(out, src):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off"] + FLAGS + [str(src), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.shim_gmres_carve_dist.restype = None
    lib.shim_gmres_carve_dist.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    return lib


def _carve(lib, nvar, n_owned, n_nodes, restart):
    out = np.zeros(18, dtype=np.int64)
    lib.shim_gmres_carve_dist(nvar, n_owned, n_nodes, restart, out.ctypes.data)
    return dict(zip(PARTS, out[:12].tolist())), out[12:].tolist()


@pytest.mark.parametrize("nvar,n_owned,n_nodes,restart", [(3, 343, 400, 30), (5, 729, 729, 30), (5, 300, 421, 1), (3, 343, 344, 128), (5, 0, 7, 30),
                                                          (5, 0, 0, 2), (5, 1685159, 1700000, 30), (5, 2 ** 27, 2 ** 27 + 5, 60)])
def test_partitioned_layout(lib, nvar, n_owned, n_nodes, restart):
    off, (nbytes, basis_bytes, partial_count, vec_blocks, stride, n) = _carve(lib, nvar, n_owned, n_nodes, restart)
    m = restart
    assert n == n_owned * nvar and stride == max(n_nodes * nvar, 1) and vec_blocks == -(-n // 1024)
    size = dict(V=(m + 1) * stride, H=(m + 1) * m, R=(m + 1) * m, cs=m, sn=m, g=m + 1, y=m, hpass=m + 1, scal=8, red=m + 2,
                partials=partial_count, rec=4)
    at = 0
    for name in PARTS:                    # in this order, one behind the other: the parts tile the allocation
        assert off[name] == at, (name, off)
        at += size[name]
    assert nbytes == 8 * at
    assert basis_bytes == 8 * (m + 1) * stride
    assert m + 2 >= (m - 1) + 2 and lib.shim_gmres_wide_max() == 130      # red holds the j + 2 sums of the last step of a cycle
    assert partial_count >= (m + 1) * vec_blocks                         # sums run over the owned entries only


@pytest.mark.parametrize("nvar,n_owned,restart", [(3, 343, 30), (5, 729, 1), (5, 0, 30)])
def test_without_n_nodes_the_layout_is_the_single_partition_one(lib, nvar, n_owned, restart):
    off, tail = _carve(lib, nvar, n_owned, -1, restart)
    off_d, tail_d = _carve(lib, nvar, n_owned, n_owned, restart)
    assert off["red"] == -1 and tail[4] == max(n_owned * nvar, 1)
    assert off_d["red"] == off["partials"] and off_d["partials"] == off["partials"] + restart + 2
    assert all(off_d[k] == off[k] for k in PARTS[:9])
    assert tail_d[0] == tail[0] + 8 * (restart + 2) and tail_d[1:] == tail[1:]


def test_stand_alone_walk_of_the_carved_state():
    """the program of tools/asan_solve_gmres_dist.sh, built here without the sanitizers: it checks its own arithmetic"""
    out = ROOT / "tests" / "_build" / "host_solve_gmres_dist_main"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_solve_gmres_dist_main.cpp"
    if _stale(out, src):
        subprocess.run(["g++", "-O1"] + FLAGS + [str(src), "-o", str(out)], check=True)
    run = subprocess.run([str(out)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr


def test_validity_rule_of_the_partitioned_entries(lib):
    """rdc_solve_state.h: rdc_solve_dist_gmres (entry DIST, gmres) records its GMRES solve as a partitioned one; the BiCGStab of
    rdc_solve_dist and the collective Arnoldi hook (entry ARNOLDI, dist) leave the record alone; no partitioned call leaves multigrid
    values that could be downloaded, the single-partition ones do"""
    SOLVE, ARNOLDI, DIST = 1, 2, 5

    def after(entry, gmres, dist):
        out = (C.c_int * 5)()
        lib.shim_valid_after(entry, gmres, dist, 30, 4, out)
        return list(out)
    assert after(DIST, 1, 0) == [0, 1, 1, 30, 4]
    assert after(DIST, 0, 0) == [0, 1, 0, 9, 1]
    assert after(ARNOLDI, 1, 1) == [0, 1, 0, 9, 1]
    assert after(ARNOLDI, 1, 0) == [1, 1, 0, 9, 1]
    assert after(SOLVE, 1, 0) == [1, 1, 0, 30, 4]
