"""GPU parity on unstructured TET4 meshes (tests/meshes.py): the five reaction-diffusion models against the oracle, per
(equation, unknown) block (tests/parity.py), on the paths SCATTER_AUTO takes on a real mesh.  On these meshes the staged
row gather (rg2) and the element-visit lists are rejected (valence > 15, tests/test_unstructured_meshes.py), so

  hydrogel, delaunay   AUTO = ROWGATHER: PIHNA / RIPF / HCC run k_tet4_rowgather, ADPM / PROTEAS k_rowgather<M, 4>,
                       with rows of more than 16 node blocks
  hub                  AUTO = COLOURED: one row exceeds a row-gather workgroup's LDS budget

and the generic evaluator (VARIANT_GENERIC) runs on every mesh, with either scatter.  The Delaunay mesh (179,455 tets)
also gives more workgroups than the device has CUs."""
import os

import numpy as np
import pytest

import meshes
from parity import assert_csr_close
from rdcfes_amd import (AssemblyContext, RdcError, adpm_params_from_dict, hcc_params_from_dict, partition,
                        pihna_params_from_dict, proteas_params_from_dict, ripf_params_from_dict, synth)
from rdcfes_amd.context import (FIELD_AUX_NODAL, FIELD_ELEM_TRACTS, FIELD_OLD_SOLUTION, SCATTER_AUTO, SCATTER_COLOURED,
                                SCATTER_ROWGATHER, VARIANT_AUTO, VARIANT_GENERIC)

pytestmark = pytest.mark.gpu
TOL = 1e-10
THREADS = max(1, min(16, len(os.sched_getaffinity(0))))
NV = {"pihna": 5, "ripf": 3, "hcc": 3, "adpm": 3, "proteas": 5}
MODELS = [("pihna", "shipped"), ("pihna", "full"), ("ripf", "shipped"), ("ripf", "full"), ("hcc", "shipped"), ("hcc", "full"),
          ("adpm", "full"), ("proteas", "full")]
AUTO_RESOLVES_TO = {"hydrogel": SCATTER_ROWGATHER, "delaunay": SCATTER_ROWGATHER, "hub": SCATTER_COLOURED}


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


_MESHES = {}


def _mesh(name, nv):
    key = (name, meshes.HUB_TETS[nv] if name == "hub" else 0)
    if key not in _MESHES:
        _MESHES[key] = meshes.hub(key[1]) if name == "hub" else getattr(meshes, name)()
    return _MESHES[key]


def _inputs(oracle, model, pv, conn, xyz, n_owned=None, fxyz=None):
    """params, fields {FIELD: array}, oracle (rp, col, val, rhs); fields from coordinates in the unit cube"""
    f = meshes.unit_cube(xyz) if fxyz is None else fxyz
    if model == "pihna":
        p = pihna_params_from_dict(synth.pihna_param_dict(pv))
        fields = {FIELD_OLD_SOLUTION: synth.pihna_fields(f)}
        ref = oracle.assemble(oracle.MODEL_PIHNA, 4, conn, xyz, 5, p, u_old=fields[FIELD_OLD_SOLUTION], n_owned=n_owned,
                              threads=THREADS)
    elif model == "ripf":
        p = ripf_params_from_dict(synth.ripf_param_dict(pv))
        u, aux = synth.ripf_fields(f)
        fields = {FIELD_OLD_SOLUTION: u, FIELD_AUX_NODAL: aux}
        ref = oracle.assemble(oracle.MODEL_RIPF, 4, conn, xyz, 3, p, u_old=u, aux=aux, n_owned=n_owned, threads=THREADS)
    elif model == "hcc":
        p = hcc_params_from_dict(synth.hcc_param_dict(pv))
        fields = {FIELD_OLD_SOLUTION: synth.hcc_fields(f)}
        ref = oracle.assemble(oracle.MODEL_HCC, 4, conn, xyz, 3, p, u_old=fields[FIELD_OLD_SOLUTION], n_owned=n_owned,
                              threads=THREADS)
    elif model == "adpm":
        p = adpm_params_from_dict(synth.adpm_param_dict(pv), time=3.0)
        u, tracts = synth.adpm_fields(f, conn.shape[0])
        fields = {FIELD_OLD_SOLUTION: u, FIELD_ELEM_TRACTS: tracts}
        ref = oracle.assemble(oracle.MODEL_ADPM, 4, conn, xyz, 3, p, u_old=u, elem_fibre=tracts, n_owned=n_owned,
                              threads=THREADS)
    else:
        p = proteas_params_from_dict(synth.proteas_param_dict(pv))
        u, aux = synth.proteas_fields(f)
        fields = {FIELD_OLD_SOLUTION: u, FIELD_AUX_NODAL: aux}
        ref = oracle.assemble(oracle.MODEL_PROTEAS, 4, conn, xyz, 5, p, u_old=u, aux=aux, n_owned=n_owned, threads=THREADS)
    return p, fields, ref


def _assemble(ctx, model, p):
    {"pihna": ctx.assemble_pihna, "ripf": ctx.assemble_ripf, "hcc": ctx.assemble_hcc, "adpm": ctx.assemble_adpm,
     "proteas": ctx.assemble_proteas}[model](p)
    return ctx.csr_download()


@pytest.mark.parametrize("mesh", ["hydrogel", "delaunay", "hub"])
@pytest.mark.parametrize("model,pv", MODELS)
def test_unstructured_parity(oracle, mesh, model, pv):
    nv = NV[model]
    conn, xyz = _mesh(mesh, nv)
    p, fields, (rp0, col0, val0, rhs0) = _inputs(oracle, model, pv, conn, xyz)
    with AssemblyContext(0) as ctx:
        ctx.mesh_upload(4, conn, xyz, nv)
        for f, a in fields.items():
            ctx.field_upload(f, a)
        rp, col = ctx.csr_pattern()
        np.testing.assert_array_equal(rp, rp0)
        np.testing.assert_array_equal(col, col0)
        for variant in (VARIANT_AUTO, VARIANT_GENERIC):
            ctx.set_kernel_variant(variant)
            for scatter in (SCATTER_AUTO, SCATTER_COLOURED):
                ctx.set_scatter(scatter)
                assert ctx.get_scatter() == (AUTO_RESOLVES_TO[mesh] if scatter == SCATTER_AUTO else SCATTER_COLOURED)
                val, rhs = _assemble(ctx, model, p)
                what = f"variant {variant}, scatter {scatter}"
                assert rel(val, val0) < TOL and rel(rhs, rhs0) < TOL, what
                try:
                    assert_csr_close(rp0, col0, val, val0, rhs, rhs0, nv)
                except AssertionError as e:
                    raise AssertionError(f"{what}: {e}") from None


@pytest.mark.parametrize("model,pv", [("pihna", "full"), ("ripf", "full"), ("hcc", "full"), ("proteas", "full")])
@pytest.mark.parametrize("scatter", [SCATTER_AUTO, SCATTER_COLOURED])
def test_unstructured_ghosted_partition(oracle, model, pv, scatter):
    """The Delaunay mesh split in two by recursive coordinate bisection: each local mesh (owned nodes first, ghost layer of
    elements) assembles the rows of its owned nodes only, against the oracle on the same local mesh and rows."""
    nv = NV[model]
    conn, xyz = _mesh("delaunay", nv)
    fxyz = meshes.unit_cube(xyz)
    part = partition.partition_rcb(xyz[conn.astype(np.int64)].mean(axis=1), 2)
    owner = partition.node_owners(conn, part, xyz.shape[0], 2)
    for rank in (0, 1):
        lp = partition.build_local(conn, xyz, part, rank, 2, owner=owner)
        assert 0 < lp.n_owned < lp.xyz.shape[0]                   # ghost nodes present
        p, fields, (rp0, col0, val0, rhs0) = _inputs(oracle, model, pv, lp.conn, lp.xyz, n_owned=lp.n_owned,
                                                     fxyz=fxyz[lp.node_global])
        with AssemblyContext(0) as ctx:
            ctx.mesh_upload(4, lp.conn, lp.xyz, nv, n_owned=lp.n_owned)
            for f, a in fields.items():
                ctx.field_upload(f, a)
            ctx.set_scatter(scatter)
            assert ctx.get_scatter() == (SCATTER_ROWGATHER if scatter == SCATTER_AUTO else SCATTER_COLOURED)
            val, rhs = _assemble(ctx, model, p)
            rp, col = ctx.csr_pattern()
        assert rhs.size == lp.n_owned * nv
        np.testing.assert_array_equal(rp, rp0)
        np.testing.assert_array_equal(col, col0)
        assert rel(val, val0) < TOL and rel(rhs, rhs0) < TOL
        assert_csr_close(rp0, col0, val, val0, rhs, rhs0, nv)


def test_more_than_256_colours_is_a_clean_error(oracle):
    """A node with more than 256 elements: rdc_mesh_upload fails with an error, and the same context then uploads and
    assembles a valid mesh correctly."""
    conn_bad, xyz_bad = meshes.hub(300)
    assert meshes.elems_per_node(conn_bad, xyz_bad.shape[0]).max() > 256
    conn, xyz = _mesh("hub", 5)
    p, fields, (rp0, col0, val0, rhs0) = _inputs(oracle, "pihna", "full", conn, xyz)
    with AssemblyContext(0) as ctx:
        with pytest.raises(RdcError, match="256 colours"):
            ctx.mesh_upload(4, conn_bad, xyz_bad, 5)
        ctx.mesh_upload(4, conn, xyz, 5)
        for f, a in fields.items():
            ctx.field_upload(f, a)
        assert ctx.get_scatter() == SCATTER_COLOURED
        val, rhs = _assemble(ctx, "pihna", p)
        rp, col = ctx.csr_pattern()
    np.testing.assert_array_equal(rp, rp0)
    np.testing.assert_array_equal(col, col0)
    assert rel(val, val0) < TOL and rel(rhs, rhs0) < TOL
    assert_csr_close(rp0, col0, val, val0, rhs, rhs0, 5)
