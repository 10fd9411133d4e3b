"""The TET4 cluster kernel (rdcfes_amd/csrc/rdc_tet4_cl.h) on the CPU, through tests/host_tet4_cl_shim.cpp:

  * the cluster lists built with cll::tet4_limits on the unstructured meshes (tests/meshes.py) and a Kuhn mesh in random
    order: every owned node in exactly one cluster, every (owned node, element) pair listed once, slots == eslot, limits
    respected (all checked inside the shim against the mesh), and the refusal of the hub mesh with its message;
  * the interior / rest split of the two-part assembly;
  * k_tet4_cl replayed on the host from those lists with the header's record gather and per-pair function, against the
    oracle: rotation, slot and offset mistakes show here without a GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import meshes
from parity import assert_csr_close
from rdcfes_amd import partition, synth
from rdcfes_amd.context import FIELD_AUX_NODAL, FIELD_ELEM_TRACTS, FIELD_OLD_SOLUTION
from test_gpu_unstructured import MODELS, NV, TOL, _inputs, rel

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rdcfes_amd" / "csrc"
STATS = ("n_wg", "n_visits", "n_pairs", "max_row", "covered", "largest", "longest", "n_blocks")
# shim model numbers: the model of the call, and the instantiations the context picks for the shipped parameter patterns
SHIM_MODEL = {"pihna": 0, "ripf": 1, "hcc": 2, "adpm": 4, "proteas": 5}
SHIM_SPECIALISED = {("pihna", "shipped"): (3, 6), ("ripf", "shipped"): (7,), ("hcc", "shipped"): (8,)}


@pytest.fixture(scope="module")
def t4():
    out = ROOT / "tests" / "_build" / "libhost_tet4_cl_shim.so"
    out.parent.mkdir(exist_ok=True)
    srcs = [ROOT / "tests" / "host_tet4_cl_shim.cpp", CSRC / "rdc_meshprep.cpp", CSRC / "rdc_prep_cl.cpp"]
    deps = srcs + list(CSRC.glob("*.h")) + [ROOT / "include" / "rdc_assembly.h"]
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                        "-Wno-unused-function", "-o", str(out)] + [str(s) for s in srcs], check=True)
    lib = C.CDLL(str(out))
    lib.t4_error.restype = C.c_char_p
    lib.t4_build.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_uint32), C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int64)]
    return lib


_MESHES = {}


def _mesh(name):
    if name not in _MESHES:
        _MESHES[name] = {"hydrogel": meshes.hydrogel, "delaunay12": lambda: meshes.delaunay(n=12), "delaunay": meshes.delaunay,
                         "kuhn6": lambda: synth.kuhn_tet_mesh(6, order="random")}[name]()
    return _MESHES[name]


def _limits(t4, nvar):
    out = (C.c_int * 4)()
    t4.t4_limits(nvar, out)
    return tuple(out)


def _build(t4, conn, n_node, n_owned, nvar, n_interior=-1, pair_order=1):
    conn = np.ascontiguousarray(conn, dtype=np.uint32)
    st = (C.c_int64 * 8)()
    rc = t4.t4_build(conn.shape[0], n_node, n_owned, conn.ctypes.data_as(C.POINTER(C.c_uint32)), nvar, n_interior, pair_order, st)
    return rc, t4.t4_error().decode(), dict(zip(STATS, list(st)))


def test_limits(t4):
    """a lane per pair of a 256-thread workgroup, a lane per element among the first 128, a half-wave per node in two rounds"""
    assert _limits(t4, 3) == (16, 256, 128, 5000)
    assert _limits(t4, 5) == (16, 256, 128, 7000)


@pytest.mark.parametrize("pair_order", [0, 1])
@pytest.mark.parametrize("nvar", [3, 5])
@pytest.mark.parametrize("mesh", ["hydrogel", "delaunay12", "delaunay", "kuhn6"])
def test_lists(t4, mesh, nvar, pair_order):
    conn, xyz = _mesh(mesh)
    n = xyz.shape[0]
    rc, err, st = _build(t4, conn, n, n, nvar, pair_order=pair_order)
    assert rc == 0, (rc, err)
    lim = _limits(t4, nvar)
    assert st["covered"] == n                                  # (exactly once each: checked in the shim)
    assert st["n_pairs"] == 4 * conn.shape[0]
    assert 1 <= st["largest"] <= lim[0] and st["max_row"] <= lim[3]
    assert st["longest"] == (meshes.valence(conn, n) + 1).max()
    assert conn.shape[0] <= st["n_visits"] <= st["n_pairs"]    # an element is gathered once per cluster that owns one of its nodes
    if mesh != "kuhn6":
        assert st["longest"] > 16                              # the rows the pair lists and the element-visit lists refuse
    # the kernel's LDS (image of the largest cluster + 128 element records) fits a CU
    out = (C.c_int64 * 4)()
    t4.t4_lds_bytes(out)
    assert max(out[:2] if nvar == 3 else out[2:]) <= 160 * 1024


@pytest.mark.parametrize("nvar", [3, 5])
def test_hub_mesh_is_refused_with_its_message(t4, nvar):
    conn, xyz = meshes.hub(meshes.HUB_TETS[nvar])
    rc, err, _ = _build(t4, conn, xyz.shape[0], xyz.shape[0], nvar)
    assert rc == 1 and err == "a row has more than 255 node blocks"


@pytest.mark.parametrize("mesh", ["delaunay12", "hydrogel"])
def test_interior_clusters_come_first(t4, mesh):
    """two-part assembly: with "interior_nodes" from a two-way RCB partition no cluster mixes interior nodes with the others, the
    interior clusters are exactly the leading ones, and no row below the reported bound belongs to a later cluster"""
    conn, xyz = _mesh(mesh)
    part = partition.partition_rcb(xyz[conn.astype(np.int64)].mean(axis=1), 2)
    for rank in (0, 1):
        lp = partition.build_local(conn, xyz, part, rank, 2)
        assert 0 < lp.n_interior < lp.n_owned < lp.xyz.shape[0]
        rc, err, st = _build(t4, lp.conn, lp.xyz.shape[0], lp.n_owned, 3, n_interior=lp.n_interior)
        assert rc == 0, (rc, err)
        assert st["covered"] == lp.n_owned and st["n_pairs"] == int((lp.conn < lp.n_owned).sum())
        out = (C.c_int64 * 3)()
        assert t4.t4_interior(out) == 0
        n_wg_int, part1_nodes, mixed = list(out)
        assert mixed == 0 and 0 < n_wg_int < st["n_wg"]
        assert 0 < part1_nodes <= lp.n_interior
        # interior_nodes = 0: an empty part 1
        rc, err, st0 = _build(t4, lp.conn, lp.xyz.shape[0], lp.n_owned, 3, n_interior=0)
        assert rc == 0 and t4.t4_interior(out) == 0 and list(out) == [0, 0, 0]
        assert st0["covered"] == lp.n_owned


def _replay(t4, model_no, p, fields, xyz, nv, n_owned, n_blocks):
    val = np.full(nv * nv * n_blocks, np.nan)
    rhs = np.full(nv * n_owned, np.nan)
    keep = [np.ascontiguousarray(a, dtype=np.float64) if a is not None else None
            for a in (xyz, fields[FIELD_OLD_SOLUTION], fields.get(FIELD_AUX_NODAL), fields.get(FIELD_ELEM_TRACTS))]
    ptr = [a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None for a in keep]
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = t4.t4_assemble(model_no, C.byref(p), ptr[0], ptr[1], ptr[2], ptr[3], dp(val), dp(rhs))
    assert rc == 0, rc
    return val, rhs


def _check(val, rhs, ref, nv, what):
    rp0, col0, val0, rhs0 = ref
    assert np.isfinite(val).all() and np.isfinite(rhs).all(), what
    assert rel(val, val0) < TOL and rel(rhs, rhs0) < TOL, what
    try:
        assert_csr_close(rp0, col0, val, val0, rhs, rhs0, nv)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


@pytest.mark.parametrize("mesh", ["hydrogel", "delaunay12"])
@pytest.mark.parametrize("model,pv", MODELS)
def test_replay_against_the_oracle(oracle, t4, mesh, model, pv):
    nv = NV[model]
    conn, xyz = _mesh(mesh)
    n = xyz.shape[0]
    p, fields, ref = _inputs(oracle, model, pv, conn, xyz)
    for order in (1, 0):
        rc, err, st = _build(t4, conn, n, n, nv, pair_order=order)
        assert rc == 0, (rc, err)
        for m in (SHIM_MODEL[model],) + (SHIM_SPECIALISED.get((model, pv), ()) if order == 1 else ()):
            val, rhs = _replay(t4, m, p, fields, xyz, nv, n, st["n_blocks"])
            _check(val, rhs, ref, nv, f"pair order {order}, shim model {m}")


def test_replay_on_a_ghosted_partition(oracle, t4):
    """owned rows only; elements may touch ghost nodes"""
    conn, xyz = _mesh("delaunay12")
    fxyz = meshes.unit_cube(xyz)
    part = partition.partition_rcb(xyz[conn.astype(np.int64)].mean(axis=1), 2)
    lp = partition.build_local(conn, xyz, part, 1, 2)
    for model, pv in (("ripf", "full"), ("proteas", "full")):
        nv = NV[model]
        p, fields, ref = _inputs(oracle, model, pv, lp.conn, lp.xyz, n_owned=lp.n_owned, fxyz=fxyz[lp.node_global])
        rc, err, st = _build(t4, lp.conn, lp.xyz.shape[0], lp.n_owned, nv, n_interior=lp.n_interior)
        assert rc == 0, (rc, err)
        val, rhs = _replay(t4, SHIM_MODEL[model], p, fields, lp.xyz, nv, lp.n_owned, st["n_blocks"])
        _check(val, rhs, ref, nv, model)
