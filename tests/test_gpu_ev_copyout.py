"""Copy-out of the element-visit kernels (evl::store_segments, rdc_ev_phases.h): one wave copies the CSR segments of two nodes with
every LDS read of both in flight -- at most four 16-byte reads per lane and segment of 25-value blocks, two of 9-value blocks --
and the moments of a block and of its mirror block are read in one batch.  Parity against the oracle as test_parity_small_mesh
asks for it, on the smallest meshes that reach every shape of a segment:

  K(3), K(4), K(6), random order   rows of 5, 7, 8, 9, 11 and 15 node blocks: 25 len (9 len) doubles with and without an odd tail, both
                                   16-byte phases, segments shorter than one wave instruction (64 x 16 bytes), clusters of at most 8 owned
                                   nodes (one image half) and of 9-16, waves with 0, 1 or 2 nodes of a half
  hub15                            K(4) and three thin tets at a boundary node of valence 6: one row of exactly 16 node blocks, the only
                                   one whose segment (400 doubles) needs the fourth 16-byte read of a lane

each with the shipped (16 moments) and the all-terms (22 moments) PIHNA parameters, through k_tet4_evq ("ev_resident" = 2; "grid" = 1:
one workgroup walks every cluster, "grid" = 3: the hand-over from the three static clusters of a workgroup to the ticket counter)
and through k_tet4_ev ("ev_resident" = 0); the all-terms RIPF model runs k_tet4_evc (9-value blocks).

K(3) has no node inside the tumour sphere of synth.pihna_fields: v is the same at every node, grad v = 0 exactly, and the blocks
(v, c) and (v, h) -- grad v times d Tau -- are exact zeros plus the rounding of sum_j v_j grad phi_j.  The oracle gives 1.0e-19 for
them next to 2.1e+10 in block (v, a) and does not reproduce them itself: with the vertices of every element rotated (the same
mesh) they change by 1.36 of their norm, every other block by less than 5e-16.  On that mesh alone they are named noise blocks of
parity.assert_csr_close, and _reference measures and asserts that spread; K(4) has 4 tumour nodes, K(6) 16, and every block is held to 1e-10."""
import ctypes as C

import numpy as np
import pytest

import meshes
from parity import assert_csr_close, block_norms
from rdcfes_amd import AssemblyContext, pihna_params_from_dict, ripf_params_from_dict, synth
from rdcfes_amd.context import FIELD_AUX_NODAL, FIELD_OLD_SOLUTION

pytestmark = pytest.mark.gpu
TOL = 1e-10          # test_gpu_parity.TOL
KUHN_VALENCES = {4, 6, 7, 8, 10, 14}

_MESHES, _ORACLE = {}, {}


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _hub15():
    """K(4), random order, and three thin tets (the cones of meshes.hub) at a boundary node of valence 6: each brings three new
    nodes, so that node has 15 neighbours -- a row of 16 node blocks -- and no node has more"""
    conn, xyz = synth.kuhn_tet_mesh(4, order="random")
    nn = xyz.shape[0]
    val = meshes.valence(conn, nn)
    boundary = np.any((np.abs(xyz) < 1e-12) | (np.abs(xyz - 1.0) < 1e-12), axis=1)
    h = int(np.flatnonzero(boundary & (val == 6))[0])
    out = (xyz[h] - 0.5) / np.linalg.norm(xyz[h] - 0.5)
    e1 = np.cross(out, [1.0, 0.0, 0.0] if abs(out[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(out, e1)
    new = []
    for w in (0.0, 2.0 * np.pi / 3.0, 4.0 * np.pi / 3.0):           # three directions 30 degrees off the outward one
        d = np.cos(np.radians(30.0)) * out + np.sin(np.radians(30.0)) * (np.cos(w) * e1 + np.sin(w) * e2)
        a1 = np.cross(d, e2 if abs(np.dot(d, e2)) < 0.9 else e1)
        a1 /= np.linalg.norm(a1)
        a2 = np.cross(d, a1)
        tip = xyz[h] + 0.5 * d
        new.append([tip + 0.012 * (np.cos(t) * a1 + np.sin(t) * a2) for t in (0.0, 2.0 * np.pi / 3.0, 4.0 * np.pi / 3.0)])
    star = np.column_stack([np.full(3, h), nn + np.arange(9).reshape(3, 3)])
    xyz2 = np.ascontiguousarray(np.vstack([xyz, np.asarray(new).reshape(-1, 3)]))
    return meshes.orient(np.vstack([conn, star]), xyz2), xyz2


def _mesh(name):
    if name not in _MESHES:
        _MESHES[name] = _hub15() if name == "hub15" else synth.kuhn_tet_mesh(int(name[1:]), order="random")
    return _MESHES[name]


def _reference(oracle, name, model, pv):
    """mesh, fields, parameters and the oracle's system: computed once per (mesh, model, parameters), never modified"""
    key = (name, model, pv)
    if key not in _ORACLE:
        conn, xyz = _mesh(name)
        if model == 0:
            p, u, aux = pihna_params_from_dict(synth.pihna_param_dict(pv)), synth.pihna_fields(xyz), None
        else:
            p = ripf_params_from_dict(synth.ripf_param_dict(pv))
            u, aux = synth.ripf_fields(xyz)
        nv = 5 if model == 0 else 3
        ref = oracle.assemble(model, 4, conn, xyz, nv, p, u_old=u, aux=aux)
        for a in ref:
            a.setflags(write=False)
        noise = ()
        if model == 0 and not u[:, [0, 1, 2, 4]].any() and np.ptp(u[:, 3]) == 0.0:
            # background state at every node (module docstring): the oracle's own spread of the two grad v blocks, on the rotated elements
            _, col1, val1, _ = oracle.assemble(0, 4, np.ascontiguousarray(conn[:, [1, 2, 0, 3]]), xyz, 5, p, u_old=u)
            np.testing.assert_array_equal(col1, ref[1])
            d, n0 = block_norms(ref[0], ref[1], val1, ref[2], 5)
            noise = ((3, 1), (3, 2))
            print(f"{name} {pv}: no tumour node; the oracle's blocks (v, c), (v, h) on rotated elements: "
                  f"{d[3, 1] / n0[3, 1]:.2e}, {d[3, 2] / n0[3, 2]:.2e} of {n0[3, 1]:.2e}, {n0[3, 2]:.2e}; largest block of the row {n0[3].max():.2e}")
            assert min(d[3, 1] / n0[3, 1], d[3, 2] / n0[3, 2]) > 1e-2 and max(n0[3, 1], n0[3, 2]) < 1e-14 * n0[3].max()
            d[3, 1] = d[3, 2] = 0.0
            assert (d <= 1e-14 * np.where(n0 > 0, n0, 1.0)).all()
        _ORACLE[key] = (conn, xyz, u, aux, p, nv, ref, noise)
    return _ORACLE[key]


def _check(oracle, name, model, pv, opts):
    conn, xyz, u, aux, p, nv, (rp0, col0, val0, rhs0), noise = _reference(oracle, name, model, pv)
    with AssemblyContext(0) as ctx:
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.mesh_upload(4, conn, xyz, nv)
        ctx.field_upload(FIELD_OLD_SOLUTION, u)
        if aux is not None:
            ctx.field_upload(FIELD_AUX_NODAL, aux)
        call = ctx.assemble_pihna if model == 0 else ctx.assemble_ripf
        call(p)
        val, rhs = ctx.csr_download()
        rp, col = ctx.csr_pattern()
        call(p)                                                      # a second assembly of the same context reproduces the first
        val2, rhs2 = ctx.csr_download()
    np.testing.assert_array_equal(rp, rp0)
    np.testing.assert_array_equal(col, col0)
    e_rhs, e_val = rel(rhs, rhs0), rel(val, val0)
    print(f"{name} model {model} {pv} {opts}: rel(rhs) {e_rhs:.3e} rel(val) {e_val:.3e} "
          f"second call {rel(val2, val):.3e} {rel(rhs2, rhs):.3e}")
    assert e_rhs < TOL
    assert e_val < TOL
    assert_csr_close(rp0, col0, val, val0, rhs, rhs0, nv, noise_blocks=noise)
    assert rel(val2, val) < 1e-13 and rel(rhs2, rhs) < 1e-13


def test_the_meshes_reach_every_row_length(shim, make_prep):
    """what the cases below rely on: the Kuhn meshes have rows of 5, 7, 8, 9, 11 and 15 node blocks, the hub mesh one node of
    exactly 15 neighbours and none of more, and its element-visit lists are built (a refusal would silently run the pair kernels)"""
    seen = set()
    for name in ("k3", "k4", "k6"):
        conn, xyz = _mesh(name)
        seen |= set(np.unique(meshes.valence(conn, xyz.shape[0])).tolist())
    assert seen == KUHN_VALENCES
    conn, xyz = _mesh("hub15")
    val = meshes.valence(conn, xyz.shape[0])
    assert val.max() == 15 and int((val == 15).sum()) == 1
    X = xyz[conn.astype(np.int64)]
    assert np.einsum("ij,ij->i", np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), X[:, 3] - X[:, 0]).min() > 0
    for nv in (5, 3):
        P = make_prep(4, conn, xyz.shape[0], xyz.shape[0], nv, lds_budget=meshes.LDS_BUDGET)
        assert P.ok, P.error
        assert P.rg2_ok                                               # the upload builds element-visit lists only behind these
        stats = (C.c_int64 * 6)()
        assert shim.shim_ev_build(C.c_int64(54000), stats) == 0, shim.shim_prep_error()


EVQ_OPTS = [{"ev_resident": 2}, {"ev_resident": 0}, {"ev_resident": 2, "grid": 1}, {"ev_resident": 2, "grid": 3}]


@pytest.mark.parametrize("opts", EVQ_OPTS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("pv", ["shipped", "full"])
@pytest.mark.parametrize("name", ["k3", "k4", "k6", "hub15"])
def test_pihna_copy_out(oracle, name, pv, opts):
    """k_tet4_evq / k_tet4_ev, 16 and 22 moments, on the state of synth.pihna_fields (background and tumour clusters)"""
    _check(oracle, name, 0, pv, opts)


@pytest.mark.parametrize("name", ["k4", "k6"])
def test_ripf_copy_out(oracle, name):
    """k_tet4_evc: segments of 9-value blocks, two 16-byte reads per lane"""
    _check(oracle, name, 1, "full", {})


@pytest.mark.parametrize("name", ["k4", "k6"])
def test_ripf_copy_out_three_workgroups_per_cu(oracle, name):
    """k_tet4_evc at the register budget of three workgroups per CU ("evc_occupancy" = 3): its copy-out takes one node at a time"""
    _check(oracle, name, 1, "full", {"evc_occupancy": 3})
