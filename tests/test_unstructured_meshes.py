"""Host list builders on the unstructured meshes of tests/test_gpu_unstructured.py (tests/meshes.py), through the shim at the
device's row-gather LDS budget.  These facts decide which kernels the GPU tests reach: a later change that gives these meshes
a fast path (rg2, element visits) or moves the COLOURED fallback has to update the GPU tests knowingly."""
import ctypes as C

import numpy as np
import pytest

import meshes


def _facts(shim, make_prep, conn, xyz, nv):
    P = make_prep(4, conn, xyz.shape[0], xyz.shape[0], nv, lds_budget=meshes.LDS_BUDGET)
    if not P.ok:
        return P, None
    stats = (C.c_int64 * 6)()
    rc = shim.shim_ev_build(C.c_int64(54000), stats)
    return P, (rc, shim.shim_prep_error())


def _positive(conn, xyz):
    X = xyz[conn.astype(np.int64)]
    v = np.einsum("ij,ij->i", np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), X[:, 3] - X[:, 0])
    return v.min() > 0


@pytest.mark.parametrize("name", ["hydrogel", "delaunay"])
@pytest.mark.parametrize("nv", [5, 3])
def test_real_meshes_take_the_row_gather_without_fast_lists(shim, make_prep, name, nv):
    conn, xyz = getattr(meshes, name)()
    assert _positive(conn, xyz)
    assert meshes.valence(conn, xyz.shape[0]).max() > 15           # rows of more than 16 node blocks
    if name == "delaunay":
        assert conn.shape[0] >= 150_000 and xyz.shape[0] == 27_000
    else:
        assert conn.shape[0] == 5504
    P, (rc, err) = _facts(shim, make_prep, conn, xyz, nv)
    assert P.ok, P.error
    assert P.rowgather_ok                                            # AUTO -> ROWGATHER
    assert not P.rg2_ok                                              # no staged row gather (k_tet4_rg5 / rg2)
    assert rc == 1 and b"16 node blocks" in err                      # no element-visit lists
    assert P.n_colours <= 256


@pytest.mark.parametrize("nv", [5, 3])
def test_hub_mesh_turns_the_row_gather_off(shim, make_prep, nv):
    """AUTO falls back to COLOURED when one row needs more than the LDS budget: the hub sizes of the GPU tests are past
    the switch (5 unknowns: between 80 and 90 hub tets, 3 unknowns: between 230 and 240) and under 256 colours."""
    lo, hi = {5: (80, 90), 3: (230, 240)}[nv]
    for n_hub, expect in ((lo, True), (hi, False), (meshes.HUB_TETS[nv], False)):
        conn, xyz = meshes.hub(n_hub)
        assert _positive(conn, xyz)
        P, (rc, err) = _facts(shim, make_prep, conn, xyz, nv)
        assert P.ok, P.error
        assert P.rowgather_ok == expect, n_hub
        assert not P.rg2_ok and rc == 1
        assert P.n_colours <= 256
    assert meshes.elems_per_node(conn, xyz.shape[0]).max() == meshes.HUB_TETS[nv] + 2


@pytest.mark.parametrize("nv", [5, 3])
def test_more_than_256_elements_at_a_node_is_an_error(shim, make_prep, nv):
    conn, xyz = meshes.hub(300)
    assert meshes.elems_per_node(conn, xyz.shape[0]).max() > 256
    P = make_prep(4, conn, xyz.shape[0], xyz.shape[0], nv, lds_budget=meshes.LDS_BUDGET)
    assert not P.ok
    assert P.error == "mesh needs more than 256 colours"
