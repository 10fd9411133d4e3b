"""tests/solve_ref_ilu_f32.py -- the numpy yardstick of the block ILU(0) with an fp32 copy of the factor (option
"ilu_factor_bits" = 32), what tests/test_gpu_solve_ilu_f32.py and tests/test_gpu_solve_ilu_f32_dist.py hold the device to --
pinned on the CPU on the oracle-assembled systems, from x0 = 0 at 1e-8 and 1e-10.  The counts are the record in DESIGN.md 7.4,
"fp32 factor": rounding the factor costs no iteration against the FP64 factor (tests/test_solve_ref_ilu.py,
tests/test_solve_ref_ilu_dist.py) on any system or world size; iterating on the fp32 operator as well costs what it costs block
Jacobi, a restart and the iterations behind it.  One rounded apply differs from the FP64 apply by 9.7e-9 .. 5.6e-8 (2-norm) on the
probe vectors of solve_ref_mg_ld."""
import numpy as np
import pytest
import scipy.sparse as sps

import solve_ref
import solve_ref_dist
import solve_ref_ilu
import solve_ref_ilu_f32
import solve_ref_mg_ld as ld
import solve_systems

TOLS = (1e-8, 1e-10)
#        system: (fp32 factor with the FP64 operator at 1e-8, 1e-10), (fp32 factor with the fp32 operator: iterations, restarts at each)
PINNED = {"pihna_kuhn": ((9, 11), ((10, 1), (14, 1))), "hcc_hex": ((5, 6), ((5, 0), (8, 1))), "solid_cube": ((18, 21), ((19, 1), (26, 1))),
          "ripf_tet": ((5, 6), ((6, 1), (8, 1))), "pihna_hydrogel": ((47, 48), ((49, 1), (87, 2))), "pihna_hub": ((7, 8), ((8, 1), (11, 1)))}
#        (system, ranks): rank-local fp32 factors, the FP64 operator
PINNED_DIST = {("pihna_kuhn", 2): (10, 12), ("pihna_kuhn", 3): (10, 13), ("hcc_hex", 2): (7, 9), ("hcc_hex", 3): (8, 10),
               ("pihna_kuhn3", 2): (6, 7), ("pihna_kuhn3", 3): (5, 7)}
_CACHE = {}


def _system(oracle, name):
    if name not in _CACHE:
        s = solve_systems.get(name)
        rp, col, val, rhs = s.oracle_assemble(oracle)
        A = sps.csr_matrix((val, col, rp), shape=(rhs.size, rhs.size))
        f = solve_ref_ilu.Factor(A, s.nv)
        _CACHE[name] = (s, A, s.rhs_scale * rhs, f, solve_ref_ilu_f32.rounded(f))
    return _CACHE[name]


@pytest.mark.parametrize("name", list(PINNED))
def test_iteration_counts(oracle, name):
    s, A, b, f, g = _system(oracle, name)
    assert f.singular == 0 and solve_ref_ilu_f32.overflows(f.F, f.diag) == 0
    plain, mixed = PINNED[name]
    for rel_tol, want, (want32, restarts32) in zip(TOLS, plain, mixed):
        x, info = solve_ref_ilu_f32.bicgstab(A, b, np.zeros(b.size), rel_tol, nv=s.nv, max_its=2000, factor=g)
        ref = solve_ref_ilu.bicgstab(A, b, np.zeros(b.size), rel_tol, nv=s.nv, max_its=2000, factor=f)[1]
        y, both = solve_ref_ilu_f32.bicgstab(A, b, np.zeros(b.size), rel_tol, nv=s.nv, max_its=2000, factor=g, mixed=True)
        print(f"{name} rel_tol {rel_tol:g}: fp32 factor {info['iterations']} iterations (restarts {info['restarts']}), FP64 factor "
              f"{ref['iterations']}; with the fp32 operator {both['iterations']} (restarts {both['restarts']})")
        for v, i in ((x, info), (y, both)):
            assert i["reason"] == solve_ref_ilu_f32.CONVERGED
            fig = solve_ref.check_solution(A, b, v, s.nv, 2, rel_tol)
            assert abs(i["residual_norm"] - fig["residual_norm"]) <= fig["rho"]
        assert info["iterations"] == want == ref["iterations"] and info["restarts"] == 0
        assert (both["iterations"], both["restarts"]) == (want32, restarts32)


@pytest.mark.parametrize("name,world", list(PINNED_DIST))
def test_iteration_counts_across_ranks(oracle, name, world):
    s, A, b = solve_ref_dist.global_system(name, oracle)
    for rel_tol, want in zip(TOLS, PINNED_DIST[(name, world)]):
        x, info = solve_ref_ilu_f32.yardstick_dist(name, world, oracle, rel_tol)
        f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
        print(f"{name} world {world} tol {rel_tol:g}: {info['iterations']} iterations (restarts {info['restarts']})")
        assert info["reason"] == solve_ref.CONVERGED and info["restarts"] == 0
        assert abs(info["residual_norm"] - f["residual_norm"]) <= f["rho"]
        assert info["iterations"] == want


@pytest.mark.parametrize("name", list(PINNED))
def test_the_rounded_apply_is_an_fp32_perturbation_of_the_apply(oracle, name):
    """between 1e-9 and 1e-6 of the FP64 apply in the 2-norm (measured: 9.7e-9 .. 5.6e-8): it differs, by what fp32 entries explain"""
    s, A, b, f, g = _system(oracle, name)
    worst, least = 0.0, np.inf
    for v in ld.probe_vectors(b.size, b):
        z, z32 = f.apply(v), g.apply(v)
        d = float(np.linalg.norm(z32 - z) / np.linalg.norm(z))
        worst, least = max(worst, d), min(least, d)
    print(f"{name}: rounded apply against the FP64 apply {least:.2e} .. {worst:.2e} (2-norm, relative)")
    assert 1e-9 <= least and worst <= 1e-6


def test_rounding_keeps_the_diagonal_blocks_and_takes_a_download(oracle):
    """blocks_of inverts csr_layout; rounded() from values() / Uinv is rounded() from the Factor; diagonal blocks stay FP64; the
    extended-precision sweeps of the rounded factor agree with the FP64 ones to FP64 noise"""
    s, A, b, f, g = _system(oracle, "pihna_kuhn")
    assert solve_ref_ilu_f32.blocks_of(f.bptr, f.values(), s.nv).tobytes() == f.F.tobytes()
    h = solve_ref_ilu_f32.rounded(f, val=f.values(), uinv=f.Uinv.reshape(-1))
    assert h.F.tobytes() == g.F.tobytes() and h.Uinv.tobytes() == g.Uinv.tobytes()
    assert g.F[f.diag].tobytes() == f.F[f.diag].tobytes()
    off = np.setdiff1d(np.arange(f.F.shape[0]), f.diag)
    assert g.F[off].tobytes() == f.F[off].astype(np.float32).astype(np.float64).tobytes() and g.F[off].tobytes() != f.F[off].tobytes()
    gl = solve_ref_ilu_f32.rounded(f, dtype=np.longdouble)
    v = np.random.default_rng(11).standard_normal(b.size)
    assert max(ld.rel_diff(g.apply(v), gl.apply(v))) <= ld.bound(64.0, 0.0)
    u = solve_ref_ilu_f32.unrounded(f, np.float64, f.values(), f.Uinv.reshape(-1))
    assert u.apply(v).tobytes() == f.apply(v).tobytes()
    big = f.F.copy()
    big[off[3], 1, 2] = 1e39
    assert solve_ref_ilu_f32.overflows(big, f.diag) == 1
