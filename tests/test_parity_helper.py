"""tests/parity.py on oracle outputs (no GPU): the per-block comparator catches what one global norm per array misses.
PIHNA on K(6) with the shipped parameters: the (v, a) block holds essentially all of the matrix norm, the n, c, h rows
about 1e-12 of it, the a-equation about 5e-11 of the rhs."""
import numpy as np
import pytest

from parity import assert_csr_close, assert_csr_close_chunked, block_norms
from rdcfes_amd import pihna_params_from_dict, synth

N, C, H, V, A = range(5)


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def global_ok(val, val0, rhs, rhs0):
    """the check every parity test made before: one relative L2 per array"""
    return rel(val, val0) < 1e-10 and rel(rhs, rhs0) < 1e-10


@pytest.fixture(scope="module")
def pihna_k6(oracle):
    conn, xyz = synth.kuhn_tet_mesh(6, order="random")
    u = synth.pihna_fields(xyz)
    p = pihna_params_from_dict(synth.pihna_param_dict("shipped"))
    rp, col, val, rhs = oracle.assemble(0, 4, conn, xyz, 5, p, u_old=u)
    return rp, col, val, rhs


def _block_mask(rp, col, a, b, nv=5):
    eq = np.repeat(np.arange(rp.size - 1) % nv, np.diff(rp))
    return (eq == a) & (col % nv == b)


def test_oracle_matches_itself(pihna_k6):
    rp, col, val0, rhs0 = pihna_k6
    assert_csr_close(rp, col, val0.copy(), val0, rhs0.copy(), rhs0, 5)
    assert_csr_close_chunked(rp, col, val0.copy(), val0, rhs0.copy(), rhs0, 5, chunk=1000)


def test_the_shares_that_make_the_global_norm_blind(pihna_k6):
    rp, col, val0, _ = pihna_k6
    _, n0 = block_norms(rp, col, val0, val0, 5)
    share = n0 / np.linalg.norm(val0)
    assert share[V, A] > 0.999
    assert share[N, N] < 1e-10 and share[C, C] < 1e-10 and share[H, H] < 1e-10
    assert share[A, N] == 0.0 and share[N, A] == 0.0             # structural zeros


def test_zeroed_nn_block(pihna_k6):
    rp, col, val0, rhs0 = pihna_k6
    val = val0.copy()
    val[_block_mask(rp, col, N, N)] = 0.0
    assert global_ok(val, val0, rhs0, rhs0)
    with pytest.raises(AssertionError, match=r"block \(0, 0\): rel error 1\.000e\+00"):
        assert_csr_close(rp, col, val, val0, rhs0, rhs0, 5)


def test_scaled_cc_block(pihna_k6):
    rp, col, val0, rhs0 = pihna_k6
    val = val0.copy()
    val[_block_mask(rp, col, C, C)] *= 1.0 + 1e-6
    assert global_ok(val, val0, rhs0, rhs0)
    with pytest.raises(AssertionError, match=r"worst matrix block \(1, 1\): rel error 1\.000e-06"):
        assert_csr_close(rp, col, val, val0, rhs0, rhs0, 5)
    with pytest.raises(AssertionError, match=r"block \(1, 1\)"):
        assert_csr_close_chunked(rp, col, val, val0, rhs0, rhs0, 5, chunk=777)


def test_perturbed_a_equation_rhs(pihna_k6):
    rp, col, val0, rhs0 = pihna_k6
    rhs = rhs0.copy()
    rhs[A::5] *= 1.0 + 1e-3
    assert global_ok(val0, val0, rhs, rhs0)
    with pytest.raises(AssertionError, match=r"rhs variable 4: rel error 1\.000e-03"):
        assert_csr_close(rp, col, val0, val0, rhs, rhs0, 5)


@pytest.mark.parametrize("factor", [0.0, -1.0, 100.0])
def test_tiny_but_resolved_ac_block(pihna_k6, factor):
    """(a, c) is 5e-17 of (a, a) but every entry is non-zero and reproducible: checked on its own norm, not as a zero"""
    rp, col, val0, rhs0 = pihna_k6
    m = _block_mask(rp, col, A, C)
    assert np.all(val0[m] != 0.0)
    _, n0 = block_norms(rp, col, val0, val0, 5)
    assert n0[A, C] < 1e-15 * n0[A, A]
    val = val0.copy()
    val[m] *= factor
    assert global_ok(val, val0, rhs0, rhs0)
    with pytest.raises(AssertionError, match=r"worst matrix block \(4, 1\): rel error"):
        assert_csr_close(rp, col, val, val0, rhs0, rhs0, 5)


@pytest.mark.parametrize("pvariant", ["shipped", "full"])
@pytest.mark.parametrize("factor", [0.0, 10.0])
def test_small_a_equation_rhs_on_the_hydrogel_mesh(oracle, pvariant, factor):
    """On the hydrogel mesh (tests/test_gpu_unstructured.py) the a-equation rhs is below 1e-16 of the v rhs: each rhs
    variable is checked on its own norm, not on the largest one"""
    import meshes
    conn, xyz = meshes.hydrogel()
    u = synth.pihna_fields(meshes.unit_cube(xyz))
    p = pihna_params_from_dict(synth.pihna_param_dict(pvariant))
    rp, col, val0, rhs0 = oracle.assemble(0, 4, conn, xyz, 5, p, u_old=u)
    r0 = np.linalg.norm(rhs0.reshape(-1, 5), axis=0)
    assert 0.0 < r0[A] < 1e-16 * r0.max()
    rhs = rhs0.copy()
    rhs[A::5] *= factor
    assert global_ok(val0, val0, rhs, rhs0)
    with pytest.raises(AssertionError, match=r"worst rhs variable 4: rel error"):
        assert_csr_close(rp, col, val0, val0, rhs, rhs0, 5)


def test_named_noise_blocks_stay_bounded(pihna_k6):
    """noise_blocks: the oracle's value is not trusted, but the block stays within 1e-14 of its equation's largest block"""
    rp, col, val0, rhs0 = pihna_k6
    _, n0 = block_norms(rp, col, val0, val0, 5)
    val = val0.copy()
    val[_block_mask(rp, col, A, C)] *= -1.0
    assert_csr_close(rp, col, val, val0, rhs0, rhs0, 5, noise_blocks={(A, C)})
    val[np.flatnonzero(_block_mask(rp, col, A, C))[0]] += 1e-13 * n0[A, A]
    with pytest.raises(AssertionError, match=r"block \(4, 1\): noise-block"):
        assert_csr_close(rp, col, val, val0, rhs0, rhs0, 5, noise_blocks={(A, C)})


def test_fill_in_of_a_structural_zero(pihna_k6):
    rp, col, val0, rhs0 = pihna_k6
    m = _block_mask(rp, col, N, A)
    assert m.any() and np.all(val0[m] == 0.0)
    val = val0.copy()
    val[np.flatnonzero(m)[7]] = 1e-6 * np.abs(val0[_block_mask(rp, col, N, N)]).max()
    assert global_ok(val, val0, rhs0, rhs0)
    with pytest.raises(AssertionError, match=r"block \(0, 4\): zero-block"):
        assert_csr_close(rp, col, val, val0, rhs0, rhs0, 5)


def test_nan_pattern_and_loosened_blocks(pihna_k6):
    rp, col, val0, rhs0 = pihna_k6
    val0n, val = val0.copy(), val0.copy()
    val0n[3] = val[3] = np.nan                                    # NaN in the same entry: left out of the norms
    assert_csr_close(rp, col, val, val0n, rhs0, rhs0, 5)
    val[4] = np.nan
    with pytest.raises(AssertionError, match="NaN pattern"):
        assert_csr_close(rp, col, val, val0n, rhs0, rhs0, 5)
    val = val0.copy()
    val[_block_mask(rp, col, C, C)] *= 1.0 + 1e-9
    with pytest.raises(AssertionError):
        assert_csr_close(rp, col, val, val0, rhs0, rhs0, 5)
    assert_csr_close(rp, col, val, val0, rhs0, rhs0, 5, block_rtol={(C, C): 1e-8})
    with pytest.raises(AssertionError, match="bug to investigate"):
        assert_csr_close(rp, col, val, val0, rhs0, rhs0, 5, block_rtol={(C, C): 1e-7})
