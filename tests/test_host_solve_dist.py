"""CPU build of rdcfes_amd/csrc/rdc_solve.h (tests/host_solve_dist_shim.cpp) for the partitioned solve: the host check of a
send list and of "interior_nodes" against the block pattern of the partitions build_local makes, the layout of the work buffer
with and without the additions of rdc_solve_dist, and the Python surface (SolveComm, solve_dist, ERR_COMM, struct size)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import solve_ref_dist
import solve_systems

ROOT = Path(__file__).resolve().parent.parent
I64P, I32P = C.POINTER(C.c_int64), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def dshim():
    out = ROOT / "tests" / "_build" / "libhost_solve_dist_shim.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "host_solve_dist_shim.cpp"
    hdr = ROOT / "rdcfes_amd" / "csrc" / "rdc_solve.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", str(src),
                        "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.shim_plan_check.argtypes = [C.c_int64, I64P, I32P, C.c_int64, C.c_int64, I32P, I64P]
    lib.shim_work_bytes.restype = C.c_int64
    lib.shim_work_bytes.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int64]
    lib.shim_work_layout.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int64, I64P, I64P]
    return lib


def _plan(lib, prep, lp, n_int, send):
    send = np.ascontiguousarray(send, dtype=np.int32)
    where = C.c_int64(-1)
    rc = lib.shim_plan_check(lp.n_owned, prep.bptr.ctypes.data_as(I64P), prep.bcol.ctypes.data_as(I32P), n_int, send.size,
                             send.ctypes.data_as(I32P), C.byref(where))
    return rc, where.value


@pytest.mark.parametrize("name,world", [("pihna_kuhn", 2), ("pihna_kuhn", 3), ("hcc_hex", 2), ("pihna_kuhn3", 3)])
def test_plan_check_on_build_local_lists(dshim, make_prep, name, world):
    s = solve_systems.pihna_kuhn(3) if name == "pihna_kuhn3" else solve_systems.get(name)
    for lp in solve_ref_dist.partitions(s, world):
        prep = make_prep(s.elem_type, lp.conn, lp.xyz.shape[0], lp.n_owned, s.nv)
        assert prep.ok, prep.error
        send = np.concatenate([lp.send_ids[q] for q in sorted(lp.send_ids)])
        assert send.size > 0
        assert _plan(dshim, prep, lp, lp.n_interior, send) == (0, -1)
        assert _plan(dshim, prep, lp, 0, send) == (0, -1)
        bad = send.copy()
        bad[bad.size // 2] = lp.n_owned                                    # a ghost, not an owned node
        assert _plan(dshim, prep, lp, lp.n_interior, bad) == (1, bad.size // 2)
        bad[bad.size // 2] = -1
        assert _plan(dshim, prep, lp, lp.n_interior, bad)[0] == 1
        if lp.n_interior < lp.n_owned:                                      # one more interior node: its row reads a ghost
            assert _plan(dshim, prep, lp, lp.n_interior + 1, send) == (3, lp.n_interior)
        assert _plan(dshim, prep, lp, lp.n_owned + 1, send)[0] == 2


def _plain_bytes(nvar, n_owned):
    """the work buffer of rdc_solve as it has been since the single-driver layout: six vectors, D^-1, partials, the scalars"""
    cdiv = lambda a, b: (a + b - 1) // b
    n = max(n_owned * nvar, 1)
    partials = max(2 * cdiv(n_owned, 16), 4 * cdiv(n_owned, 256), 3 * cdiv(n_owned * nvar, 1024)) + 8
    return (6 * n + n * nvar + partials) * 8 + 80


@pytest.mark.parametrize("nvar", [3, 5])
def test_plain_work_buffer_is_unchanged(dshim, nvar):
    for n_owned in (0, 1, 15, 16, 17, 255, 256, 257, 729, 1024, 4097, 1728000):
        assert dshim.shim_work_bytes(nvar, n_owned, 0, 0, 0, 0) == _plain_bytes(nvar, n_owned), n_owned


@pytest.mark.parametrize("nvar,n_owned,n_nodes,n_int,n_send", [
    (5, 405, 486, 324, 81), (5, 324, 405, 243, 81), (5, 180, 270, 108, 140), (3, 196, 245, 147, 49), (5, 8, 40, 0, 8),
    (5, 729, 729, 0, 0), (3, 1, 2, 1, 1), (5, 33, 34, 17, 3), (5, 100000, 104000, 95999, 5000), (3, 0, 5, 0, 0)])
def test_dist_work_buffer_layout(dshim, nvar, n_owned, n_nodes, n_int, n_send):
    out = (C.c_int64 * 22)()
    need = C.c_int64()
    for dist in (1, 0):
        k = dshim.shim_work_layout(nvar, n_owned, dist, n_nodes, n_int, n_send, out, C.byref(need))
        assert k == (11 if dist else 9)
        total = dshim.shim_work_bytes(nvar, n_owned, dist, n_nodes, n_int, n_send)
        spans = [(out[2 * i], out[2 * i + 1]) for i in range(k)]
        names = ["r", "rh", "p", "v", "s", "t", "dinv", "partials"] + (["send", "rec"] if dist else []) + ["scal"]
        for i, (off, size) in enumerate(spans):
            end = spans[i + 1][0] if i + 1 < k else total
            if names[i] == "partials":
                size = end - off                                           # as large as the gap; must hold the largest set
                assert size >= 8 * need.value, (size, need.value)
            assert 0 <= off and off + size <= end <= total, (names[i], off, size, end, total)
            assert off % 8 == 0
        assert spans == sorted(spans)
        if dist:   # p and s can receive their ghosts; the two ranges' partials fit
            assert spans[2][1] == spans[4][1] == 8 * n_nodes * nvar
            cdiv = lambda a, b: (a + b - 1) // b
            assert need.value >= 2 * (cdiv(n_int, 16) + cdiv(n_owned - n_int, 16))
    assert dshim.shim_work_bytes(nvar, n_owned, 0, 0, 0, 0) == _plain_bytes(nvar, n_owned)


def test_python_surface():
    import rdcfes_amd
    from rdcfes_amd import AssemblyContext, ERR_COMM, SolveComm, halo, params
    assert ERR_COMM == 6
    assert callable(AssemblyContext.solve_dist) and callable(AssemblyContext.solve_dist_plan)
    assert SolveComm is halo.SolveComm and "SolveComm" in rdcfes_amd.__all__ and "ERR_COMM" in rdcfes_amd.__all__
    assert C.sizeof(params.SolveCommStruct) == 32
    assert [f[0] for f in params.SolveCommStruct._fields_] == ["user", "exchange_begin", "exchange_end", "allreduce_sum"]


def test_solve_comm_lists_follow_build_local():
    """send list in peer order, per-peer slices of the send buffer and of the ghost tail; both sides of a pair agree"""
    from rdcfes_amd import SolveComm
    s = solve_systems.get("pihna_kuhn")
    lps = solve_ref_dist.partitions(s, 3)
    comms = [SolveComm(lp, s.nv, "cpu") for lp in lps]
    for lp, c in zip(lps, comms):
        assert c.world == 1 and not c.host_staged
        assert c.n_ghost == lp.xyz.shape[0] - lp.n_owned and c.bytes_per_exchange == 8 * s.nv * c.n_send
        assert c.send_nodes.dtype == np.int32 and np.all(c.send_nodes < lp.n_owned)
        covered = np.zeros(c.n_ghost, dtype=int)
        for q, (a, b) in c.recv_slice.items():
            covered[a:b] += 1
            sa, sb = comms[q].send_slice[lp.rank]
            # what q sends me, in q's order, are the nodes I receive, in mine
            assert np.array_equal(lps[q].node_global[comms[q].send_nodes[sa:sb]], lp.node_global[lp.n_owned + a:lp.n_owned + b])
        assert np.all(covered == 1)
