"""The reference's own example inputs for the reaction-diffusion models (run/PIHNA, run/RIPF133, run/HCP102513,
run/Coupled/HCC): the `input.dat` parameter files and the initial nodal field files are fixtures under tests/golden/
(data; the field files gzip-compressed, contents unchanged).  The reference ships no expected outputs and none of the
meshes of these four cases, so these tests check
  (i)   that the parameter structs the kernels receive for the "shipped" variants of the benchmarks (rdcfes_amd.synth)
        are exactly what the files say, read the way each model's input() reads them;
  (ii)  the facts about the field files the synthetic fields are modelled on;
  (iii) (gpu) HIP == oracle with the SHIPPED nodal states on a stand-in mesh of the same size -- the degenerate
        initial states a real run starts from (uniform vasculature with 23 seed nodes; fb = 0 everywhere;
        PrP = 1 with 62 seeded nodes), which the random benchmark states never produce."""
import ctypes as C
import gzip
from pathlib import Path

import numpy as np
import pytest

from parity import assert_csr_close, block_norms
from rdcfes_amd import (RipfCheckParams, adpm_params_from_dict, hcc_params_from_dict, inputs, pihna_params_from_dict,
                        ripf_params_from_dict, synth)
from rdcfes_amd import params as P

G = Path(__file__).parent / "golden"
TOL = 1e-10


def _bytes(s):
    return bytes(memoryview(s))


def _field(name, ncol):
    a = np.array(gzip.decompress((G / name).read_bytes()).split(), dtype=np.float64)
    assert a.size % ncol == 0
    return a.reshape(-1, ncol)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------
# (i) parameter files
# ---------------------------------------------------------------------------------------------------------------------
def test_pihna_input_is_the_shipped_variant():
    d = inputs.read_model_input(G / "run_PIHNA_input.dat", P.PIHNA_KEYS)
    assert d == synth.pihna_param_dict("shipped")
    assert _bytes(pihna_params_from_dict(d)) == _bytes(pihna_params_from_dict(synth.pihna_param_dict("shipped")))
    # the specialised kernel's conditions: integer exponent 3, no cell transport, no uptake
    assert d["cells_max_capacity/exponent"] == 3.0 and d["diffuse/c"] == d["taxis/c"] == d["diffuse/h"] == d["taxis/h"] == 0.0
    assert d["taxis/v"] == 0.0 and d["uptake/a/from/v"] == 0.0 and d["diffuse/v"] == 0.5


def test_ripf_input_is_the_shipped_variant():
    d = inputs.read_model_input(G / "run_RIPF133_input.dat", P.RIPF_KEYS)
    want = synth.ripf_param_dict("shipped")
    run_time = {"RT_dose/total/max": want.pop("RT_dose/total/max")}      # set by check_solution, not by the file (:771)
    zeros = {k: v for k, v in d.items() if k not in want}                # keys the file spells out with their default
    assert zeros == {"HU/phi/cc/build": 0.0, "HU/phi/cc/decay": 0.0, "HU/phi/fb/build": 0.0, "HU/phi/fb/decay": 0.0}
    assert {k: d[k] for k in want} == want
    assert "cc/kappa" not in d                                           # commented out in the file: default 0
    a, b = ripf_params_from_dict({**d, **run_time}), ripf_params_from_dict(synth.ripf_param_dict("shipped"))
    assert _bytes(a) == _bytes(b)
    assert a.VolFr_max_vacant == 1.0 - 1.0e-5                            # src/ripf.C:180-182


def test_ripf_total_dose_of_the_shipped_plan(oracle):
    """`RT_dose/total/max` = 73 in the benchmarks is what check_solution (src/ripf.C:697-771) leaves after the last
    fraction of the shipped plan: max(broad + focus) = 73.73, stored through an int parameter."""
    kv = inputs.parse_getpot((G / "run_RIPF133_input.dat").read_text())
    nb, nf = int(kv["RT_dose/broad/fractions"]), int(kv["RT_dose/focus/fractions"])
    assert (nb, nf, float(kv["HU/min"]), float(kv["HU/max"])) == (28, 8, -1000.0, 1000.0)
    u = _field("run_RIPF133_Lung_Model_Initial_Nodal_Field.dat.gz", 3)
    rt2 = _field("run_RIPF133_Lung_Model_Initial_Nodal_Field~RT.dat.gz", 2)
    rt = np.column_stack([rt2, np.zeros(rt2.shape[0])])
    for day, expect in ((0, rt2[:, 0] / nb), (nb, rt2[:, 1] / nf + rt2[:, 0]), (nb + nf, rt2.sum(1))):
        p = RipfCheckParams(float(kv["time_step"]), float(kv["HU/min"]), float(kv["HU/max"]), nb, nf, day, 0)
        s, pv, td, r, aux, mx = oracle.ripf_check_solution(p, u, u, rt)
        np.testing.assert_allclose(r[:, 2], expect, rtol=1e-15)
        assert mx == expect.max()
        # the clamp touches the shipped state: HU runs to -1019 and +1094 in the file
        assert s[:, 0].min() == -1000.0 and s[:, 0].max() == 1000.0 and (u[:, 0] < -1000).sum() > 0 and (u[:, 0] > 1000).sum() > 0
    assert int(mx) == synth.ripf_param_dict("shipped")["RT_dose/total/max"] == 73


def test_adpm_input_is_the_shipped_variant():
    """The file's `taxis/A_b`, `taxis/Tau` (+ pulse) keys are not names input() asks for (src/adpm.C:194-199,216-221
    read `taxis_1/...`, `taxis_2/...`): they drop out and the shipped run has no taxis."""
    kv = inputs.parse_getpot((G / "run_HCP102513_input.dat").read_text())
    d = inputs.model_keys(kv, P.ADPM_KEYS)
    assert d == synth.adpm_param_dict("shipped")
    assert {"taxis/A_b", "taxis/A_b/pulse/0", "taxis/Tau", "taxis/Tau/pulse/1"} <= set(kv) and not any(k.startswith("taxis") for k in d)
    for t in (0.0, 3.0):
        assert _bytes(adpm_params_from_dict(d, time=t)) == _bytes(adpm_params_from_dict(synth.adpm_param_dict("shipped"), time=t))
    p = adpm_params_from_dict(d)
    assert list(p.taxis1_A_b) == [0.0, -1.0e-20, 1.0e20] and list(p.decay_PrP) == [1.0e-4, 0.01, 10.0]
    assert list(p.decay_Tau) == [10.0, 0.0005, 1.0e20]                   # pulse/1 not in the file: default


def test_hcc_input_is_the_shipped_variant():
    path = G / "run_Coupled_HCC_input.dat"
    d = inputs.read_model_input(path, P.HCC_KEYS)
    assert d == synth.hcc_param_dict("shipped")                          # capacity keys only: every rate is 0
    assert _bytes(hcc_params_from_dict(d)) == _bytes(hcc_params_from_dict(synth.hcc_param_dict("shipped")))
    s = inputs.read_solid_input(path)                                    # same keys as src/solid.C (src/coupled_hcc.C:308-346)
    assert s.penalty == 1.0e8 and s.use_symmetry is False                # `solver/use_symmetry` is not the key read
    assert sorted(s.bcs) == [2000, 2002, 2003] and s.bcs[2000] == (0.0, 0.0, 0.0)
    assert np.isnan(s.bcs[2002][0]) and np.isnan(s.bcs[2003][1]) and s.bcs[2002][2] == 0.0     # NaN = free component
    assert sorted(s.materials) == [3000, 3001, 3002]
    for m, rate in ((3000, 0.0), (3001, 0.0), (3002, 0.3)):
        mat = s.materials[m]
        assert (mat.Young, mat.Poisson, mat.FibreStiffness, tuple(mat.rate)) == (2.0e3, 0.4, 0.0, (rate,) * 3)


# ---------------------------------------------------------------------------------------------------------------------
# (ii) field files
# ---------------------------------------------------------------------------------------------------------------------
def test_pihna_nodal_file_facts():
    a = _field("run_PIHNA_Brain_Model_Initial_Nodal_Field.dat.gz", 5)    # n c h v a, src/pihna.C:287-292
    assert a.shape == (24903, 5)
    assert np.all(a[:, 3] == 7170.0) and np.all(a[:, [0, 2, 4]] == 0.0)
    assert set(np.unique(a[:, 1])) == {0.0, 1000.0} and int((a[:, 1] == 1000.0).sum()) == 23
    bg = synth.pihna_fields(np.full((4, 3), 0.99))                      # outside the synthetic tumour sphere
    assert np.all(bg == a[0])


def test_ripf_nodal_file_facts():
    u = _field("run_RIPF133_Lung_Model_Initial_Nodal_Field.dat.gz", 3)   # HU cc fb, src/ripf.C:317
    rt = _field("run_RIPF133_Lung_Model_Initial_Nodal_Field~RT.dat.gz", 2)   # broad focus, src/ripf.C:278
    assert u.shape == (15700, 3) and rt.shape == (15700, 2)
    assert (u[:, 0].min(), u[:, 0].max()) == (-1019.0, 1094.0)
    assert (u[:, 1].min(), u[:, 1].max()) == (0.0, 1.0) and int((u[:, 1] > 0).sum()) == 537 and np.all(u[:, 2] == 0.0)
    assert rt.min() == 0.0 and rt[:, 0].max() == 67.0 and abs(rt[:, 1].max() - 6.732893) < 1e-12
    su, _ = synth.ripf_fields(np.random.default_rng(0).uniform(0, 1, (4000, 3)))
    assert -1019.0 <= su[:, 0].min() and su[:, 0].max() <= 1094.0 and 0.0 <= su[:, 1].min() and su[:, 1].max() <= 1.0


def test_adpm_nodal_file_facts():
    a = _field("run_HCP102513_Brain_Model_Initial_Nodal_Field.dat.gz", 3)    # PrP A_b Tau, src/adpm.C:284
    assert a.shape == (25935, 3) and np.all(a[:, 0] == 1.0)
    for v in (1, 2):
        assert set(np.unique(a[:, v])) == {0.0, 0.01} and int((a[:, v] > 0).sum()) == 62


def test_field_reader_on_a_shipped_file(tmp_path):
    from rdcfes_amd import io
    raw = gzip.decompress((G / "run_PIHNA_Brain_Model_Initial_Nodal_Field.dat.gz").read_bytes())
    (tmp_path / "f.dat").write_bytes(raw)
    a = io.read_field_dat(tmp_path / "f.dat", 24903, 5)
    np.testing.assert_array_equal(a, _field("run_PIHNA_Brain_Model_Initial_Nodal_Field.dat.gz", 5))
    with pytest.raises(ValueError):
        io.read_field_dat(tmp_path / "f.dat", 24904, 5)                 # a mesh with more nodes than the file has rows


# ---------------------------------------------------------------------------------------------------------------------
# (iii) HIP == oracle on the shipped initial states
# ---------------------------------------------------------------------------------------------------------------------
def _assemble(model, conn, xyz, nv, p, u, aux=None, tracts=None, options=()):
    from rdcfes_amd import AssemblyContext, FIELD_AUX_NODAL, FIELD_ELEM_TRACTS, FIELD_OLD_SOLUTION
    with AssemblyContext(0) as ctx:
        for k, v in options:
            ctx.set_option(k, v)
        ctx.mesh_upload(4, conn, xyz, nv)
        ctx.field_upload(FIELD_OLD_SOLUTION, u)
        if aux is not None:
            ctx.field_upload(FIELD_AUX_NODAL, aux)
        if tracts is not None:
            ctx.field_upload(FIELD_ELEM_TRACTS, tracts)
        getattr(ctx, "assemble_" + model)(p)
        return ctx.csr_download()


@pytest.mark.gpu
@pytest.mark.parametrize("options", [(), (("moments", 0),), (("kernel", 1),)])
def test_gpu_pihna_shipped_initial_state(oracle, options):
    """K(28) = 131,712 TET4 / 24,389 nodes stands in for the missing 134,646 / 24,903 brain mesh; node i takes one of
    the file's last 24,389 rows (all 23 seeded rows are among them).  In this state Te = 7170 / 2.39e5 on all but the
    seeded elements, a = 0 everywhere (the cytokine terms multiply 0) and c jumps 0 -> 1000 across one element."""
    a = _field("run_PIHNA_Brain_Model_Initial_Nodal_Field.dat.gz", 5)
    conn, xyz = synth.kuhn_tet_mesh(28, order="random")
    u = np.ascontiguousarray(a[-xyz.shape[0]:])
    assert int((u[:, 1] == 1000.0).sum()) == 23
    p = pihna_params_from_dict(inputs.read_model_input(G / "run_PIHNA_input.dat", P.PIHNA_KEYS))
    rp0, col0, val0, rhs0 = oracle.assemble(oracle.MODEL_PIHNA, 4, conn, xyz, 5, p, u_old=u, threads=8)
    val, rhs = _assemble("pihna", conn, xyz, 5, p, u, options=options)
    assert rel(rhs, rhs0) < TOL and rel(val, val0) < TOL
    # (v, c) and (v, h) are exact zeros plus rounding in this state: 6.1e-28 of the (v, a) block.  The oracle does not
    # reproduce them itself -- the same assembly with the elements reversed and their vertices rotated differs by 1.30
    # of their norm there (2e-16 to 6e-16 in every other block) -- and the kernels measured 1.33 to 1.37.  Held to 1e-14
    # of (v, a) as noise; the spread is asserted so that a state in which they become resolved drops the exemption.
    _, _, val1, _ = oracle.assemble(oracle.MODEL_PIHNA, 4, np.ascontiguousarray(conn[::-1][:, [1, 2, 0, 3]]), xyz, 5, p,
                                    u_old=u, threads=8)
    spread, n0 = block_norms(rp0, col0, val1, val0, 5)
    noise = {(3, 1), (3, 2)}
    assert all(spread[b] > 1e-2 * n0[b] and n0[b] < 1e-20 * n0[3].max() for b in noise)
    assert_csr_close(rp0, col0, val, val0, rhs, rhs0, 5, noise_blocks=noise)
    # rows of a node whose element patch is all background: Fe_n = Fe_c = Fe_h = Fe_a = 0 (nothing to produce from)
    seeded = np.zeros(xyz.shape[0], bool)
    seeded[np.unique(conn[np.isin(conn, np.nonzero(u[:, 1])[0]).any(1)])] = True
    quiet = rhs.reshape(-1, 5)[~seeded]
    assert np.all(quiet[:, [0, 1, 2, 4]] == 0.0) and np.all(quiet[:, 3] > 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("day", [0, 36])
def test_gpu_ripf_shipped_initial_state(oracle, day):
    """K(24) = 82,944 TET4 / 15,625 nodes for the 15,700-node lung mesh; the dose record is what check_solution leaves
    on `day` of the shipped plan, the rates are 0 (first step).  fb = 0 everywhere: grad fb = 0, so the haptotaxis
    blocks vanish and the unit radiotherapy gradient is the only direction in the element."""
    from rdcfes_amd import AssemblyContext, FIELD_AUX_NODAL, FIELD_OLD_SOLUTION, FIELD_PREV_SOLUTION, FIELD_RT_DOSE
    conn, xyz = synth.kuhn_tet_mesh(24, order="random")
    n = xyz.shape[0]
    u = np.ascontiguousarray(_field("run_RIPF133_Lung_Model_Initial_Nodal_Field.dat.gz", 3)[:n])
    rt2 = _field("run_RIPF133_Lung_Model_Initial_Nodal_Field~RT.dat.gz", 2)[:n]
    rt = np.ascontiguousarray(np.column_stack([rt2, np.zeros(n)]))
    ck = RipfCheckParams(0.1, -1000.0, 1000.0, 28, 8, day, 0)
    s0, _, _, _, aux0, mx0 = oracle.ripf_check_solution(ck, u, u, rt)
    d = inputs.read_model_input(G / "run_RIPF133_input.dat", P.RIPF_KEYS)
    with AssemblyContext(0) as ctx:
        ctx.mesh_upload(4, conn, xyz, 3)
        ctx.field_upload(FIELD_OLD_SOLUTION, u)
        ctx.field_upload(FIELD_PREV_SOLUTION, u)
        ctx.field_upload(FIELD_RT_DOSE, rt)
        mx = ctx.ripf_check_solution(ck)
        assert abs(mx - mx0) <= 1e-15 * mx0
        p = ripf_params_from_dict({**d, "RT_dose/total/max": int(mx)})
        ctx.assemble_ripf(p)
        val, rhs = ctx.csr_download()
        np.testing.assert_array_equal(ctx.field_download(FIELD_OLD_SOLUTION, 3 * n).reshape(n, 3), s0)
    rp0, col0, val0, rhs0 = oracle.assemble(oracle.MODEL_RIPF, 4, conn, xyz, 3, p, u_old=s0, aux=aux0, threads=8)
    assert rel(rhs, rhs0) < TOL and rel(val, val0) < TOL
    assert_csr_close(rp0, col0, val, val0, rhs, rhs0, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("time", [0.0, 3.0])
def test_gpu_adpm_shipped_initial_state(oracle, time):
    """K(29) = 146,334 TET4 / 27,000 nodes for the 125,702-element / 25,935-node brain mesh (rows repeat cyclically for
    the last 1,065 nodes); the 3.5 MB tract file is not a fixture, the tracts are synthetic with its magnitude."""
    a = _field("run_HCP102513_Brain_Model_Initial_Nodal_Field.dat.gz", 3)
    conn, xyz = synth.kuhn_tet_mesh(29, order="random")
    u = np.ascontiguousarray(np.resize(a, (xyz.shape[0], 3)))
    _, tracts = synth.adpm_fields(xyz, conn.shape[0])
    p = adpm_params_from_dict(inputs.read_model_input(G / "run_HCP102513_input.dat", P.ADPM_KEYS), time=time)
    rp0, col0, val0, rhs0 = oracle.assemble(oracle.MODEL_ADPM, 4, conn, xyz, 3, p, u_old=u, elem_fibre=tracts, threads=8)
    val, rhs = _assemble("adpm", conn, xyz, 3, p, u, tracts=tracts)
    assert rel(rhs, rhs0) < TOL and rel(val, val0) < TOL
    assert_csr_close(rp0, col0, val, val0, rhs, rhs0, 3)
