"""ADPM assembly (src/adpm.C:324-652), SURVEY §8(f) rank 3: oracle KATs, product row code vs oracle on the host,
HIP vs oracle on the GPU."""
import numpy as np
import pytest

from conftest import shim_rows
from parity import assert_csr_close
from rdcfes_amd import adpm_params_from_dict, synth


def _elem(nen, seed, variant="full", time=2.0):
    rng = np.random.default_rng(seed)
    if nen == 4:
        X = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float) + 0.15 * rng.standard_normal((4, 3))
    else:
        X = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], float)
        X = X + 0.08 * rng.standard_normal((8, 3))
    u = np.column_stack([rng.uniform(0.5, 1.5, nen), rng.uniform(0.0, 0.02, nen), rng.uniform(0.0, 0.02, nen)])
    t = 0.1 * rng.standard_normal(3)
    return X, u, t, adpm_params_from_dict(synth.adpm_param_dict(variant), time=time)


def _mass(oracle, nen, X):
    phi, dphi, jxw = oracle.fe_reinit(nen, X)
    return np.einsum("q,qi,qj->ij", jxw, phi, phi)


@pytest.mark.parametrize("nen", [4, 8])
def test_oracle_zero_rates_give_mass_matrix(oracle, nen):
    X, u, t, _ = _elem(nen, 1)
    p = adpm_params_from_dict({"time_step": 0.05})
    Ke, Fe = oracle.element(oracle.MODEL_ADPM, nen, X, u, p, elem_data=t)
    M = _mass(oracle, nen, X)
    for a in range(3):
        for b in range(3):
            blk = Ke[a * nen:(a + 1) * nen, b * nen:(b + 1) * nen]
            np.testing.assert_allclose(blk, M if a == b else 0.0, atol=1e-15)
        np.testing.assert_allclose(Fe[a * nen:(a + 1) * nen], M @ u[:, a], rtol=1e-13)


@pytest.mark.parametrize("nen", [4, 8])
def test_oracle_linearisation(oracle, nen):
    """Ke = M - dt/2 * df/du and Fe = M u + dt/2 * f(u)  =>  Ke + dFe/du = 2M wherever the piecewise rates
    and the tract choice do not switch inside the finite-difference step -- except the two columns upstream
    leaves out: d/dTau of the A_b taxis_2 gate and d/dA_b of the Tau one are zero a.e. anyway (Pi_ is piecewise
    constant), so the identity holds for every block."""
    clean = 0
    for seed in range(6):
        X, u, t, p = _elem(nen, 10 + seed)
        Ke, Fe = oracle.element(oracle.MODEL_ADPM, nen, X, u, p, elem_data=t)
        M = _mass(oracle, nen, X)
        J = np.zeros_like(Ke)
        h = 1e-7
        for b in range(3):
            for j in range(nen):
                up, um = u.copy(), u.copy()
                up[j, b] += h; um[j, b] -= h
                Fp = oracle.element(oracle.MODEL_ADPM, nen, X, up, p, elem_data=t)[1]
                Fm = oracle.element(oracle.MODEL_ADPM, nen, X, um, p, elem_data=t)[1]
                J[:, b * nen + j] = (Fp - Fm) / (2 * h)
        M3 = np.kron(np.eye(3), M)
        err = np.abs(Ke + J - 2 * M3).max() / np.abs(M3).max()
        # a rate or tract choice switching inside +-h shows up as an O(1) error (rare seeds, skipped);
        # anything in between would be a wrong derivative
        if err < 1e-5:
            clean += 1
        else:
            assert err > 1e-2, f"seed {seed}: inconsistent linearisation, error {err}"
    assert clean >= 4


@pytest.mark.parametrize("nen", [4, 8])
@pytest.mark.parametrize("variant", ["shipped", "full"])
def test_product_rows_match_oracle(oracle, shim, nen, variant):
    for seed in range(6):
        X, u, t, p = _elem(nen, 30 + seed, variant)
        Ke0, Fe0 = oracle.element(oracle.MODEL_ADPM, nen, X, u, p, elem_data=t)
        s = np.abs(Ke0).max()
        for fast in ((False, True) if nen == 4 else (False,)):   # generic quadrature-loop row / factored TET4 row
            Ke1, Fe1 = shim_rows(shim, 4, nen, p, X, u, elem_data=t, fast=fast)
            np.testing.assert_allclose(Ke1, Ke0, rtol=1e-10, atol=1e-13 * s)
            np.testing.assert_allclose(Fe1, Fe0, rtol=1e-10, atol=1e-13 * np.abs(Fe0).max())


def test_tract_selection(oracle):
    """tract = +-t when the unit gradient is within the angle of +-t, else 0 (src/adpm.C:477-493): with
    taxis_1 only and a uniform A_b gradient along x the taxis block is +-, or vanishes, with t."""
    X = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float)
    u = np.column_stack([np.ones(4), 0.01 + 0.005 * X[:, 0], np.full(4, 0.01)])
    d = {"time_step": 0.1, "taxis/A_b/angle": 30.0, "taxis_1/A_b": 1.0, "taxis_1/A_b/pulse/0": 0.0, "taxis_1/A_b/pulse/1": 1.0}
    p = adpm_params_from_dict(d)
    base = oracle.element(oracle.MODEL_ADPM, 4, X, u, adpm_params_from_dict({"time_step": 0.1}), elem_data=[1, 0, 0])[1]
    f_al = oracle.element(oracle.MODEL_ADPM, 4, X, u, p, elem_data=[1.0, 0.0, 0.0])[1] - base
    f_op = oracle.element(oracle.MODEL_ADPM, 4, X, u, p, elem_data=[-1.0, 0.0, 0.0])[1] - base
    f_pp = oracle.element(oracle.MODEL_ADPM, 4, X, u, p, elem_data=[0.0, 1.0, 0.0])[1] - base
    assert np.abs(f_al[4:8]).max() > 0 and np.allclose(f_al, f_op) and np.abs(f_pp).max() == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("nen,n", [(4, 5), (8, 4)])
@pytest.mark.parametrize("variant", ["shipped", "full"])
@pytest.mark.parametrize("scatter", [1, 2])
@pytest.mark.parametrize("kernel_variant", [0, 1])   # 0 = auto (factored TET4 kernels), 1 = generic evaluator
def test_gpu_parity(oracle, nen, n, variant, scatter, kernel_variant):
    from rdcfes_amd import AssemblyContext, FIELD_ELEM_TRACTS, FIELD_OLD_SOLUTION
    conn, xyz = synth.kuhn_tet_mesh(n, jitter=0.1, order="random") if nen == 4 else synth.hex_mesh(n, jitter=0.1, order="random")
    u, tracts = synth.adpm_fields(xyz, conn.shape[0])
    p = adpm_params_from_dict(synth.adpm_param_dict(variant), time=3.0)
    rp0, col0, val0, rhs0 = oracle.assemble(oracle.MODEL_ADPM, nen, conn, xyz, 3, p, u_old=u, elem_fibre=tracts)
    with AssemblyContext(0) as ctx:
        ctx.set_kernel_variant(kernel_variant)
        ctx.mesh_upload(nen, conn, xyz, 3)
        ctx.field_upload(FIELD_OLD_SOLUTION, u)
        with pytest.raises(Exception):
            ctx.assemble_adpm(p)                  # tracts not set
        ctx.field_upload(FIELD_ELEM_TRACTS, tracts)
        ctx.set_scatter(scatter)
        ctx.assemble_adpm(p)
        val, rhs = ctx.csr_download()
    assert np.linalg.norm(rhs - rhs0) <= 1e-10 * np.linalg.norm(rhs0)
    assert np.linalg.norm(val - val0) <= 1e-10 * np.linalg.norm(val0)
    assert_csr_close(rp0, col0, val, val0, rhs, rhs0, 3)
