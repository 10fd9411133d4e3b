"""The reference's own shipped solid cases (run/Solid/uniaxial_compression, run/Solid/hydrogel_tension):
its Gmsh meshes and input.dat files are the fixtures under tests/golden/ (data, copied unchanged).  The
reference holds no expected outputs for them, so these tests check (i) the readers against facts of the
files, (ii) known-answer properties of the oracle on them, (iii) HIP == oracle on them (gpu)."""
from pathlib import Path

import numpy as np
import pytest

from parity import assert_csr_close
from rdcfes_amd import gmsh, inputs

G = Path(__file__).parent / "golden"
CASES = {
    "cube": (G / "solid_uniaxial_compression_cube.msh", G / "solid_uniaxial_compression_input.dat"),
    "hydrogel": (G / "solid_hydrogel_tension_model.msh", G / "solid_hydrogel_tension_input.dat"),
}
TOL = 1e-10


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _signed_volumes(mesh):
    X = mesh.xyz[mesh.conn.astype(np.int64)]
    if mesh.elem_type == 4:
        return np.einsum("ei,ei->e", X[:, 1] - X[:, 0], np.cross(X[:, 2] - X[:, 0], X[:, 3] - X[:, 0])) / 6.0
    # HEX8: Jacobian at the centroid (trilinear map), exact volume for parallelepipeds
    xi = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]]) / 8.0
    J = np.einsum("nk,end->ekd", xi, X)
    return 8.0 * np.linalg.det(J)


def test_read_cube():
    m = gmsh.read_msh2(CASES["cube"][0])
    assert m.elem_type == 8 and m.conn.shape == (512, 8) and m.xyz.shape == (729, 3)
    assert m.face_nodes.shape == (384, 4) and sorted(np.unique(m.face_tag)) == [0, 1, 2, 3, 4, 5]
    assert np.all(m.subdomain == 0)
    v = _signed_volumes(m)
    assert np.all(v > 0)                       # libMesh needs positively oriented elements
    ext = m.xyz.max(0) - m.xyz.min(0)
    assert abs(v.sum() - ext.prod()) < 1e-9 * ext.prod()
    for bid in range(6):                       # every tagged face is a side of exactly one element
        e, s = m.sides_with_boundary_id(bid)
        assert e.size == 64 and np.unique(e * 6 + s).size == 64


def test_read_hydrogel():
    m = gmsh.read_msh2(CASES["hydrogel"][0])
    assert m.elem_type == 4 and m.conn.shape == (5504, 4)
    assert m.face_nodes.shape[1] == 3 and set(np.unique(m.face_tag)) == {0, 1, 2, 6, 10}
    assert np.all(_signed_volumes(m) > 0)
    assert np.unique(m.conn).size == m.xyz.shape[0]      # no orphan nodes
    n = sum(m.sides_with_boundary_id(b)[0].size for b in (0, 1, 2, 6, 10))
    assert n == m.face_nodes.shape[0]


def test_input_semantics():
    """The shipped keys `material/0/Neohookean/*` and `solver/use_symmetry` are not the ones read
    (src/solid.C:236,268-272): the coded defaults apply."""
    s = inputs.read_solid_input(CASES["cube"][1])
    assert s.loading_step == 0.1 and s.n_load_steps == 10 and s.penalty == 1.0e8 and not s.use_symmetry
    assert sorted(s.bcs) == [0, 5] and s.bcs[0] == (0.0, 0.0, 0.0)
    assert np.isnan(s.bcs[5][0]) and np.isnan(s.bcs[5][1]) and s.bcs[5][2] == -0.75
    m = s.materials[0]
    assert (m.Young, m.Poisson, m.FibreStiffness) == (1.0e3, 0.3, 0.0)
    h = inputs.read_solid_input(CASES["hydrogel"][1])
    assert sorted(h.bcs) == [0, 1, 2, 10] and h.bcs[10] == (-0.001, 0.0, 0.0) and h.materials[0].Young == 1.0e3
    kv = inputs.parse_getpot("a = 1 # c\n#b = 2\ns = ' 1 2 '\nmaterial/0/Hyperelastic/Young = 5.\n")
    assert kv == {"a": "1", "s": " 1 2 ", "material/0/Hyperelastic/Young": "5."}
    assert inputs.SolidSetup(kv).materials[0].Young == 5.0


def _case(name, pseudo_time, amp):
    mesh = gmsh.read_msh2(CASES[name][0])
    setup = inputs.read_solid_input(CASES[name][1])
    em, mats = setup.material_table(mesh.subdomain)
    Xu = mesh.xyz
    L = (Xu.max(0) - Xu.min(0)).max()
    rng = np.random.default_rng(5)
    x = Xu + amp * L * (0.05 * np.sin(3.0 * Xu / L + 0.3) + 0.002 * rng.standard_normal(Xu.shape))
    fibre = np.tile([0.0, 0.0, 1.0], (mesh.conn.shape[0], 1))
    return mesh, setup, em, mats, Xu, x, fibre, setup.sides(mesh), setup.params(pseudo_time)


@pytest.mark.parametrize("name", ["cube", "hydrogel"])
def test_oracle_known_answers(oracle, name):
    """Undeformed state: zero internal force, so the residual is the penalty term alone,
    R = -penalty * sum_sides int (x - X - ratio*ubar) phi_i  (src/solid_system.C:291-330) — its component
    sums are  penalty * ratio * ubar_d * area(boundary)  on the constrained directions and 0 on NaN ones;
    the Jacobian is symmetric and (without the penalty) annihilates rigid translations."""
    mesh, setup, em, mats, Xu, _, fibre, sides, sp = _case(name, 0.3, 0.0)
    nen = mesh.elem_type
    rp, col, val, rhs = oracle.assemble(oracle.MODEL_SOLID, nen, mesh.conn, Xu, 3, sp, xyz_undeformed=Xu, elem_fibre=fibre,
                                       elem_material=em, materials=mats, sides=sides)
    import scipy.sparse as sps
    n = 3 * Xu.shape[0]
    ratio = 0.3 * 1.000001
    expect = np.zeros(3)
    for bcid, disp in setup.bcs.items():
        f = mesh.face_nodes[mesh.face_tag == bcid]
        P = Xu[f]
        if f.shape[1] == 3:
            area = 0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1).sum()
        else:
            area = (0.5 * np.linalg.norm(np.cross(P[:, 2] - P[:, 0], P[:, 3] - P[:, 1]), axis=1)).sum()
        for d in range(3):
            if not np.isnan(disp[d]):
                expect[d] += setup.penalty * ratio * disp[d] * area
    got = rhs.reshape(-1, 3).sum(0)
    scale = max(np.abs(expect).max(), 1.0)
    # sign convention of the oracle follows the reference's residual: compare magnitudes per direction
    assert np.allclose(np.abs(got), np.abs(expect), rtol=1e-9, atol=1e-9 * scale)
    # nodes off the constrained boundary carry no force in the undeformed state
    on = np.zeros(Xu.shape[0], bool)
    for bcid in setup.bcs:
        on[np.unique(mesh.face_nodes[mesh.face_tag == bcid])] = True
    assert np.abs(rhs.reshape(-1, 3)[~on]).max() < 1e-9 * scale
    if rp is not None:
        A = sps.csr_matrix((val, col, rp), shape=(n, n))
        assert abs(A - A.T).max() < 1e-9 * abs(A).max()
        # without penalty rows: K * (rigid translation) = 0
        sp0 = setup.params(0.3)
        _, _, v0, _ = oracle.assemble(oracle.MODEL_SOLID, nen, mesh.conn, Xu, 3, sp0, xyz_undeformed=Xu, elem_fibre=fibre,
                                      elem_material=em, materials=mats)
        K = sps.csr_matrix((v0, col, rp), shape=(n, n))
        t = np.tile([1.0, -2.0, 0.5], Xu.shape[0])
        assert np.abs(K @ t).max() < 1e-9 * abs(K).max()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube", "hydrogel"])
@pytest.mark.parametrize("jac", [True, False])
def test_gpu_parity_on_shipped_case(oracle, name, jac):
    from rdcfes_amd import AssemblyContext, FIELD_ELEM_FIBRE, FIELD_UNDEFORMED_XYZ
    mesh, setup, em, mats, Xu, x, fibre, sides, sp = _case(name, 0.4, 1.0)
    nen = mesh.elem_type
    rp0, col0, val0, rhs0 = oracle.assemble(oracle.MODEL_SOLID, nen, mesh.conn, x, 3, sp, xyz_undeformed=Xu, elem_fibre=fibre,
                                            elem_material=em, materials=mats, request_jacobian=jac, sides=sides)
    with AssemblyContext(0) as ctx:
        ctx.mesh_upload(nen, mesh.conn, x, 3)
        ctx.field_upload(FIELD_UNDEFORMED_XYZ, Xu)
        ctx.field_upload(FIELD_ELEM_FIBRE, fibre)
        ctx.solid_set_materials(em, mats)
        ctx.solid_set_sides(*sides)
        ctx.solid_assemble(sp, jac)
        val, rhs = ctx.csr_download()
    assert rel(rhs, rhs0) < TOL
    if jac:
        assert rel(val, val0) < TOL
        assert_csr_close(rp0, col0, val, val0, rhs, rhs0, 3)


def test_oracle_regression(oracle):
    """Drift guard: the oracle still produces the committed outputs (made by make_oracle_regression.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mk", G / "make_oracle_regression.py")
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    gold = np.load(G / "oracle_regression.npz")
    for k, (val, rhs) in mk.cases().items():
        assert rel(val, gold[k + "_val"]) < 1e-13, k
        assert rel(rhs, gold[k + "_rhs"]) < 1e-13, k
