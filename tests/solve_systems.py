"""The linear systems the solver tests run on, each described once for the oracle (CPU yardstick) and for an
AssemblyContext (GPU): name -> System.  All single-partition; `ghosted_pihna()` gives the one partitioned case.
At the end: what every GPU solve test does with one of them (_dev, _open, _unchanged)."""
import copy
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np
import scipy.sparse as sps

import meshes
from rdcfes_amd import (AssemblyContext, gmsh, hcc_params_from_dict, inputs, partition, pihna_params_from_dict, ripf_params_from_dict, synth)

G = Path(__file__).resolve().parent / "golden"
FIELD_OLD_SOLUTION, FIELD_AUX_NODAL, FIELD_UNDEFORMED_XYZ, FIELD_ELEM_FIBRE = 0, 1, 2, 3


@dataclass
class System:
    name: str
    model: str                 # pihna | ripf | hcc | solid
    elem_type: int
    conn: np.ndarray
    xyz: np.ndarray
    nv: int
    params: object
    fields: dict               # FIELD id -> array
    rhs_scale: float = 1.0
    n_owned: int = None
    solid: dict = field(default_factory=dict)   # em, mats, sides

    def oracle_assemble(self, O, u_old=None):
        """(row_ptr, col, val, rhs) from the oracle; u_old overrides the old solution (time loop)"""
        u = self.fields.get(FIELD_OLD_SOLUTION) if u_old is None else u_old
        if self.model == "solid":
            return O.assemble(O.MODEL_SOLID, self.elem_type, self.conn, self.xyz, 3, self.params,
                              xyz_undeformed=self.fields[FIELD_UNDEFORMED_XYZ], elem_fibre=self.fields[FIELD_ELEM_FIBRE],
                              elem_material=self.solid["em"], materials=self.solid["mats"], sides=self.solid["sides"])
        model = {"pihna": O.MODEL_PIHNA, "ripf": O.MODEL_RIPF, "hcc": O.MODEL_HCC}[self.model]
        return O.assemble(model, self.elem_type, self.conn, self.xyz, self.nv, self.params, u_old=u,
                          aux=self.fields.get(FIELD_AUX_NODAL), n_owned=self.n_owned)

    def upload(self, ctx):
        ctx.mesh_upload(self.elem_type, self.conn, self.xyz, self.nv, n_owned=self.n_owned)
        for f, a in self.fields.items():
            ctx.field_upload(f, a)
        if self.model == "solid":
            ctx.solid_set_materials(self.solid["em"], self.solid["mats"])
            ctx.solid_set_sides(*self.solid["sides"])

    def assemble(self, ctx):
        if self.model == "solid":
            ctx.solid_assemble(self.params, True)
        else:
            {"pihna": ctx.assemble_pihna, "ripf": ctx.assemble_ripf, "hcc": ctx.assemble_hcc}[self.model](self.params)


def _pihna(name, conn, xyz, fxyz=None, n_owned=None):
    u = synth.pihna_fields(xyz if fxyz is None else fxyz)
    return System(name, "pihna", 4, conn, xyz, 5, pihna_params_from_dict(synth.pihna_param_dict("shipped")),
                  {FIELD_OLD_SOLUTION: u}, n_owned=n_owned)


def pihna_kuhn(n=8):
    conn, xyz = synth.kuhn_tet_mesh(n, order="random")
    return _pihna(f"pihna_kuhn{n}", conn, xyz)


def haptotaxis_cfl_time_step(conn, xyz, hu, d):
    """largest time step with a cell Courant number of 1 for the transport of fb: min over the tets of
    h_e / (haptotaxis |grad HU|_e + radiotaxis), h_e the shortest edge (the radiotherapy gradient enters as a unit vector)"""
    c = conn.astype(np.int64)
    X = xyz[c]
    g = np.linalg.solve(X[:, 1:] - X[:, :1], (hu[c][:, 1:] - hu[c][:, :1])[..., None])[..., 0]
    edges = np.linalg.norm(X[:, :, None] - X[:, None, :], axis=-1)
    h = np.where(edges > 0, edges, np.inf).min(axis=(1, 2))
    return float((h / (d["fb/haptotaxis"] * np.linalg.norm(g, axis=1) + d.get("fb/radiotaxis", 0.0))).min())


def ripf_tet(cfl=True):
    """RIPF, all terms on, K(6).  The fb equation transports fb along grad HU with a diffusion of 1e-3; synth.ripf_fields
    draws HU per node from [-1019, 1094], |grad HU| up to 2e4 on this mesh.  At the shipped time_step 0.1 the cell Courant
    number of that transport is about 900 and the Galerkin matrix is indefinite (negative diagonal entries in the fb rows):
    no Jacobi-class Krylov method is meant for that regime.  The solver case therefore takes the time step from the state,
    Courant number 1 (haptotaxis_cfl_time_step: 1.09e-4 here), a criterion evaluated before any solve; cfl=False keeps
    the shipped 0.1 (matvec, and the test that a solve which does not converge says so)."""
    conn, xyz = synth.kuhn_tet_mesh(6, order="random")
    u, aux = synth.ripf_fields(xyz)
    d = synth.ripf_param_dict("full")
    if cfl:
        d["time_step"] = haptotaxis_cfl_time_step(conn, xyz, u[:, 0], d)
    return System("ripf_tet" if cfl else "ripf_tet_dt01", "ripf", 4, conn, xyz, 3, ripf_params_from_dict(d),
                  {FIELD_OLD_SOLUTION: u, FIELD_AUX_NODAL: aux})


def ripf_tet_dt01():
    return ripf_tet(cfl=False)


def _hcc(name, et, conn, xyz):
    return System(name, "hcc", et, conn, xyz, 3, hcc_params_from_dict(synth.hcc_param_dict("full")),
                  {FIELD_OLD_SOLUTION: synth.hcc_fields(xyz)})


def hcc_tet():
    return _hcc("hcc_tet", 4, *synth.kuhn_tet_mesh(6, order="random"))


def hcc_hex():
    return _hcc("hcc_hex", 8, *synth.hex_mesh(6, jitter=0.1, order="random"))


def solid_cube():
    mesh = gmsh.read_msh2(G / "solid_uniaxial_compression_cube.msh")
    setup = inputs.read_solid_input(G / "solid_uniaxial_compression_input.dat")
    em, mats = setup.material_table(mesh.subdomain)
    fibre = np.tile([0.0, 0.0, 1.0], (mesh.conn.shape[0], 1))
    return System("solid_cube", "solid", 8, mesh.conn, mesh.xyz, 3, setup.params(0.1),
                  {FIELD_UNDEFORMED_XYZ: mesh.xyz, FIELD_ELEM_FIBRE: fibre}, rhs_scale=-1.0,
                  solid=dict(em=em, mats=mats, sides=setup.sides(mesh)))


def pihna_hydrogel():
    conn, xyz = meshes.hydrogel()
    return _pihna("pihna_hydrogel", conn, xyz, fxyz=meshes.unit_cube(xyz))


def pihna_hub():
    conn, xyz = meshes.hub(max(meshes.HUB_TETS.values()))   # the largest hub tests/test_gpu_unstructured.py uploads (245 tets): one row of 740 blocks
    return _pihna("pihna_hub", conn, xyz, fxyz=meshes.unit_cube(xyz))


def ghosted_pihna():
    """rank 0 of a two-way split of K(8): owned nodes first, a ghost layer behind them"""
    conn, xyz = synth.kuhn_tet_mesh(8, order="random")
    part = partition.partition_rcb(xyz[conn.astype(np.int64)].mean(axis=1), 2)
    owner = partition.node_owners(conn, part, xyz.shape[0], 2)
    lp = partition.build_local(conn, xyz, part, 0, 2, owner=owner)
    assert 0 < lp.n_owned < lp.xyz.shape[0]
    return _pihna("pihna_ghosted", lp.conn, lp.xyz, n_owned=lp.n_owned)


SOLVE_SYSTEMS = {"pihna_kuhn": pihna_kuhn, "ripf_tet": ripf_tet, "hcc_tet": hcc_tet, "hcc_hex": hcc_hex, "solid_cube": solid_cube,
                 "pihna_hydrogel": pihna_hydrogel, "pihna_hub": pihna_hub}
MATVEC_SYSTEMS = dict(SOLVE_SYSTEMS, ripf_tet_dt01=ripf_tet_dt01, pihna_ghosted=ghosted_pihna)
_CACHE = {}


def get(name):
    if name not in _CACHE:
        _CACHE[name] = MATVEC_SYSTEMS[name]()
    return _CACHE[name]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _open(name, params=None):
    """uploaded + assembled context, the system (with `params` in place of its own), A (owned rows x all local dofs),
    assembled rhs, raw values"""
    s = get(name)
    if params is not None:
        s = copy.copy(s)
        s.params = params
    ctx = AssemblyContext(0)
    s.upload(ctx)
    s.assemble(ctx)
    val, rhs = ctx.csr_download()
    rp, col = ctx.csr_pattern()
    A = sps.csr_matrix((val, col, rp), shape=(rhs.size, ctx.n_node * s.nv))
    return ctx, s, A, rhs, val


def _unchanged(ctx, val, rhs):
    v, r = ctx.csr_download()
    assert v.tobytes() == val.tobytes() and r.tobytes() == rhs.tobytes(), "CSR values / rhs were modified"
