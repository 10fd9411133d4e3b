"""The TET4 cluster kernel k_tet4_cl (rdc_tet4_cluster_mode, rdcfes_amd/csrc/rdc_tet4_cl.hip) on the GPU: parity with the oracle
per (equation, unknown) block on the unstructured meshes of tests/meshes.py, where mode 1 replaces the row-gather kernels, and
on a Kuhn mesh, where mode 2 forces it.  Every case asserts the path through tet4_cluster_info()["active"]: none may pass
by a silent fall-back."""
import numpy as np
import pytest

import meshes
from parity import assert_csr_close
from rdcfes_amd import AssemblyContext, RdcError, hcc_params_from_dict, partition, synth
from rdcfes_amd.context import (ERR_INVALID, FIELD_OLD_SOLUTION, SCATTER_AUTO, SCATTER_COLOURED, SCATTER_ROWGATHER, VARIANT_AUTO,
                                VARIANT_GENERIC)
from test_gpu_unstructured import MODELS, NV, TOL, _assemble, _inputs, rel

pytestmark = pytest.mark.gpu
FULL = [("pihna", "full"), ("ripf", "full"), ("hcc", "full"), ("adpm", "full"), ("proteas", "full")]

_MESHES = {}


def _mesh(name, nv=0):
    key = (name, meshes.HUB_TETS[nv] if name == "hub" else 0)
    if key not in _MESHES:
        _MESHES[key] = {"hydrogel": meshes.hydrogel, "delaunay12": lambda: meshes.delaunay(n=12), "delaunay": meshes.delaunay,
                        "kuhn6": lambda: synth.kuhn_tet_mesh(6, order="random"), "hub": lambda: meshes.hub(key[1])}[name]()
    return _MESHES[key]


def _check(val, rhs, ref, nv, what=""):
    rp0, col0, val0, rhs0 = ref
    assert np.isfinite(val).all() and np.isfinite(rhs).all(), what
    assert rel(val, val0) < TOL and rel(rhs, rhs0) < TOL, what
    try:
        assert_csr_close(rp0, col0, val, val0, rhs, rhs0, nv)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


def _upload(ctx, conn, xyz, nv, fields, n_owned=None):
    ctx.mesh_upload(4, conn, xyz, nv, n_owned=n_owned)
    for f, a in fields.items():
        ctx.field_upload(f, a)


def _pattern_equal(ctx, ref):
    rp, col = ctx.csr_pattern()
    np.testing.assert_array_equal(rp, ref[0])
    np.testing.assert_array_equal(col, ref[1])


def _active_info(ctx, conn, n_owned):
    """the info of a call that launched the kernel: the lists describe the mesh, the launch had LDS"""
    info = ctx.tet4_cluster_info()
    assert info["active"] == 1, info
    assert info["n_pairs"] == int((conn < n_owned).sum())
    assert 0 < info["n_clusters"] <= n_owned and conn.shape[0] <= info["n_elem_visits"] <= info["n_pairs"]
    assert 0 < info["lds_bytes"] <= 160 * 1024
    return info


@pytest.mark.parametrize("mesh", ["hydrogel", "delaunay12"])
@pytest.mark.parametrize("model,pv", MODELS)
def test_mode1_small_meshes(oracle, mesh, model, pv):
    nv = NV[model]
    conn, xyz = _mesh(mesh)
    p, fields, ref = _inputs(oracle, model, pv, conn, xyz)
    with AssemblyContext(0) as ctx:
        assert ctx.tet4_cluster_info()["mode"] == 0 and ctx.tet4_cluster_info()["n_clusters"] == 0
        ctx.set_tet4_cluster(1)                                   # before the upload
        _upload(ctx, conn, xyz, nv, fields)
        _pattern_equal(ctx, ref)
        assert ctx.get_scatter() == SCATTER_ROWGATHER
        val, rhs = _assemble(ctx, model, p)
        info = _active_info(ctx, conn, xyz.shape[0])
        assert info["mode"] == 1
        _check(val, rhs, ref, nv)


@pytest.mark.parametrize("model,pv", FULL)
def test_mode1_more_clusters_than_cus(oracle, model, pv):
    """meshes.delaunay(): 3,816 clusters, rows of up to 50 node blocks"""
    nv = NV[model]
    conn, xyz = _mesh("delaunay")
    p, fields, ref = _inputs(oracle, model, pv, conn, xyz)
    with AssemblyContext(0) as ctx:
        _upload(ctx, conn, xyz, nv, fields)
        ctx.set_tet4_cluster(1)                                   # after the upload
        val, rhs = _assemble(ctx, model, p)
        assert _active_info(ctx, conn, xyz.shape[0])["n_clusters"] > 1024
        _pattern_equal(ctx, ref)
        _check(val, rhs, ref, nv)


@pytest.mark.parametrize("model,pv", MODELS)
def test_mode2_on_a_kuhn_mesh_and_back(oracle, model, pv):
    """mode 1 leaves a mesh with pair lists alone, mode 2 forces the cluster kernel, mode 0 switches back: same context"""
    nv = NV[model]
    conn, xyz = _mesh("kuhn6")
    p, fields, ref = _inputs(oracle, model, pv, conn, xyz)
    with AssemblyContext(0) as ctx:
        _upload(ctx, conn, xyz, nv, fields)
        ctx.set_tet4_cluster(1)
        val, rhs = _assemble(ctx, model, p)
        assert ctx.tet4_cluster_info()["active"] == 0
        _check(val, rhs, ref, nv, "mode 1")
        ctx.set_tet4_cluster(2)
        val, rhs = _assemble(ctx, model, p)
        _active_info(ctx, conn, xyz.shape[0])
        _check(val, rhs, ref, nv, "mode 2")
        ctx.set_tet4_cluster(0)
        val, rhs = _assemble(ctx, model, p)
        info = ctx.tet4_cluster_info()
        assert info["active"] == 0 and info["lds_bytes"] == 0 and info["n_clusters"] > 0    # the lists stay, the path is off
        _check(val, rhs, ref, nv, "mode 0")


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("model,pv", [("pihna", "full"), ("hcc", "full")])
def test_hub_mesh_falls_back(oracle, model, pv, mode):
    """a row of more than 255 node blocks: the lists are refused, the scatter resolves as before, the builder's reason is kept"""
    nv = NV[model]
    conn, xyz = _mesh("hub", nv)
    p, fields, ref = _inputs(oracle, model, pv, conn, xyz)
    with AssemblyContext(0) as ctx:
        ctx.set_tet4_cluster(mode)
        _upload(ctx, conn, xyz, nv, fields)
        assert ctx.get_scatter() == SCATTER_COLOURED
        val, rhs = _assemble(ctx, model, p)
        info = ctx.tet4_cluster_info()
        assert info["active"] == 0 and info["n_clusters"] == 0 and info["mode"] == mode
        assert info["last_error"] == "a row has more than 255 node blocks"
        assert ctx.get_scatter() == SCATTER_COLOURED
        _check(val, rhs, ref, nv)


@pytest.mark.parametrize("model,pv", [("pihna", "shipped"), ("ripf", "full")])
def test_overrides_keep_their_paths(oracle, model, pv):
    nv = NV[model]
    conn, xyz = _mesh("delaunay12")
    p, fields, ref = _inputs(oracle, model, pv, conn, xyz)
    with AssemblyContext(0) as ctx:
        ctx.set_tet4_cluster(2)
        _upload(ctx, conn, xyz, nv, fields)
        for variant, scatter, active in ((VARIANT_GENERIC, SCATTER_AUTO, 0), (VARIANT_AUTO, SCATTER_COLOURED, 0),
                                         (VARIANT_AUTO, SCATTER_ROWGATHER, 1), (VARIANT_AUTO, SCATTER_AUTO, 1)):
            ctx.set_kernel_variant(variant)
            ctx.set_scatter(scatter)
            val, rhs = _assemble(ctx, model, p)
            assert ctx.tet4_cluster_info()["active"] == active, (variant, scatter)
            _check(val, rhs, ref, nv, f"variant {variant}, scatter {scatter}")


_LOCAL = {}


def _local(rank):
    """delaunay(n=12) in two ranks by recursive coordinate bisection: the local mesh of `rank` and its field coordinates"""
    if not _LOCAL:
        conn, xyz = _mesh("delaunay12")
        fxyz = meshes.unit_cube(xyz)
        part = partition.partition_rcb(xyz[conn.astype(np.int64)].mean(axis=1), 2)
        owner = partition.node_owners(conn, part, xyz.shape[0], 2)
        for r in (0, 1):
            lp = partition.build_local(conn, xyz, part, r, 2, owner=owner)
            assert 0 < lp.n_interior < lp.n_owned < lp.xyz.shape[0]
            _LOCAL[r] = (lp, fxyz[lp.node_global])
    return _LOCAL[rank]


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("model,pv", FULL)
def test_ghosted_contexts(oracle, model, pv, rank):
    """owned rows only; the clusters hold owned nodes, their elements touch ghosts"""
    nv = NV[model]
    lp, fxyz = _local(rank)
    p, fields, ref = _inputs(oracle, model, pv, lp.conn, lp.xyz, n_owned=lp.n_owned, fxyz=fxyz)
    with AssemblyContext(0) as ctx:
        ctx.set_tet4_cluster(1)
        _upload(ctx, lp.conn, lp.xyz, nv, fields, n_owned=lp.n_owned)
        val, rhs = _assemble(ctx, model, p)
        _active_info(ctx, lp.conn, lp.n_owned)
        _pattern_equal(ctx, ref)
    assert rhs.size == lp.n_owned * nv
    _check(val, rhs, ref, nv)


@pytest.mark.parametrize("interior", ["partition", "none"])
@pytest.mark.parametrize("model,pv", [("pihna", "shipped"), ("pihna", "full"), ("hcc", "full")])
def test_two_part_assembly(oracle, model, pv, interior):
    """part 1 (the interior clusters) on a second stream, then part 2: the rows below part1_nodes() are complete after part 1
    (downloaded before part 2 runs), the two parts together are the whole assembly.  interior_nodes = 0: an empty part 1"""
    import torch
    nv = NV[model]
    lp, fxyz = _local(0)
    p, fields, ref = _inputs(oracle, model, pv, lp.conn, lp.xyz, n_owned=lp.n_owned, fxyz=fxyz)
    part = {"pihna": AssemblyContext.assemble_pihna_part, "hcc": AssemblyContext.assemble_hcc_part}[model]
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    n_int = lp.n_interior if interior == "partition" else 0
    with AssemblyContext(0) as ctx:
        ctx.set_option("interior_nodes", n_int)
        ctx.set_tet4_cluster(1)
        _upload(ctx, lp.conn, lp.xyz, nv, fields, n_owned=lp.n_owned)
        ctx.field_upload(FIELD_OLD_SOLUTION, 0.5 * fields[FIELD_OLD_SOLUTION])      # every row holds something else first
        _assemble(ctx, model, p)
        assert ctx.tet4_cluster_info()["active"] == 1
        ctx.field_upload(FIELD_OLD_SOLUTION, fields[FIELD_OLD_SOLUTION])
        val, rhs = np.full_like(ref[2], np.nan), np.full_like(ref[3], np.nan)
        part(ctx, p, 1, side.cuda_stream)
        n1 = ctx.part1_nodes()
        side.synchronize()
        if interior == "partition":
            assert ctx.tet4_cluster_info()["active"] == 1
            assert 0 < n1 <= n_int
        else:
            assert ctx.tet4_cluster_info()["active"] == 0 and n1 == 0             # RDC_OK without a launch
        ctx.csr_download_rows(0, n1, val.ctypes.data, rhs.ctypes.data)
        part(ctx, p, 2)
        assert ctx.tet4_cluster_info()["active"] == 1
        ctx.csr_download_rows(n1, lp.n_owned, val.ctypes.data, rhs.ctypes.data)
    _check(val, rhs, ref, nv)


def test_mode_values(oracle):
    with AssemblyContext(0) as ctx:
        for bad in (3, -1):
            with pytest.raises(RdcError) as ei:
                ctx.set_tet4_cluster(bad)
            assert ei.value.code == ERR_INVALID
            assert ctx.tet4_cluster_info()["mode"] == 0
        # a HEX8 mesh: accepted, no effect
        conn, xyz = synth.hex_mesh(5, jitter=0.1, order="random")
        u = synth.hcc_fields(xyz)
        p = hcc_params_from_dict(synth.hcc_param_dict("full"))
        ref = oracle.assemble(oracle.MODEL_HCC, 8, conn, xyz, 3, p, u_old=u)
        ctx.set_tet4_cluster(2)
        ctx.mesh_upload(8, conn, xyz, 3)
        ctx.field_upload(FIELD_OLD_SOLUTION, u)
        ctx.assemble_hcc(p)
        info = ctx.tet4_cluster_info()
        assert info["mode"] == 2 and info["active"] == 0 and info["n_clusters"] == 0 and info["lds_bytes"] == 0
        val, rhs = ctx.csr_download()
        _check(val, rhs, ref, 3)
